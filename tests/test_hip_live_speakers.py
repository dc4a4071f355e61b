"""Every face of a recording or live stream in one audio pass (AVNet.open_streams(speakers=K) / SpeakerStreamPool,
AVNet.separate_long_speakers, System.open_camera_streams(speakers=K), rtfs_live_ingest_frame_speakers_f32, rtfs_live_reset_speakers_f32,
rtfs_longform_frame_speakers_f32) against tests/live_speakers_oracle.py:

1. framing is a copy: every tick's audio and video windows bit-equal to the oracle's, K = 2 and 3, over the plans of
   tests/test_hip_live.py, three slots (two ring wraps / one frame-short flush / one short window), chunk tensors 4 bytes into their
   allocation, the K tracks once as K allocations and once as one (K,512,m) tensor with identical results; the long-form launch too;
2. the overlap-add launch with n_src = K against the float64 streaming oracle at test_hip_longform.ola_bound, hop == window bit-equal;
3. composition with the real separator: == oracle overlap-add of separate_speakers on the chunks the schedule lists (ola_bound), ==
   separate_long per face of the whole recording (tests/util.rel_err <= 1e-4); separate_long_speakers against separate_long per track;
4. the camera pool against System.separate_recording per face, the lip embeddings bit-equal to video_model on the whole track;
5. slot reuse after flush and after reset, bit-equal to a fresh pool;
6. refusals on device tensors launch nothing and leave no trace;
7. the cases again in child processes on poisoned memory (RTFS_POISON_WS = nan, big)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.params import make_inputs
from tests import live_oracle as VO
from tests import live_speakers_oracle as SO
from tests import live_video_oracle as LV
from tests.test_hip_live import MODES, PLANS, Sized, offset_view
from tests.test_hip_longform import dev, host, lib, model, ola_bound
from tests.util import rel_err

pytestmark = pytest.mark.gpu

SPF = 640
POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")


def open_pool(K, **kw):
    from rtfs_net_amd import streaming
    return streaming.open_speaker_streams(Sized(model(4), 1), speakers=K, **kw)


def drive(pool, xs, vs, events, window, hop, max_chunk, y_of=None, stacked=False):
    """Stream recordings xs[s] (L,) with lips vs[s] (K,512,Tv) through slot s by ``events``; chunk tensors start 4 bytes into their
    allocation, the K tracks of a chunk as K allocations or (``stacked``) as one (K,512,m) tensor.  With ``y_of`` (row-wise function of
    the framed windows, numpy) the separator is replaced: every tick's framed windows are compared bit for bit against the oracle, and
    the outputs against the float64 streaming overlap-add at ola_bound.  Returns slot -> concatenated (K, L) output, worst error / bound."""
    K = pool.speakers
    counters = {s: (0, 0, 0, 0) for s in xs}
    pos = {s: [0, 0] for s in xs}
    olas = {s: SO.OverlapAdd(window, hop, K) for s in xs}
    got = {s: [] for s in xs}
    y_max = {s: 0.0 for s in xs}
    seen = {}

    def fake_forward(rows):
        seen["xw"], seen["vw"] = host(pool._xw[:rows]).copy(), host(pool._vw[:rows * K]).copy()
        seen["y"] = y_of(seen["xw"], seen["vw"], K).astype(np.float32)
        pool._y[:rows].copy_(dev(seen["y"]))

    if y_of is not None:
        pool._forward_rows = fake_forward
    worst = 0.0
    for kind, ids, na, nf in events:
        flush = kind == "flush"
        want = SO.tick(counters, ids, na, nf, window, hop, max_chunk, K, flush)
        if flush:
            outs = pool.flush(ids)
        else:
            wavs = [offset_view(xs[s][pos[s][0]:pos[s][0] + n]) for s, n in zip(ids, na)]
            cut = [np.ascontiguousarray(vs[s][:, :, pos[s][1]:pos[s][1] + n]) for s, n in zip(ids, nf)]
            vids = [offset_view(c) for c in cut] if stacked else [[offset_view(c[k]) for k in range(K)] for c in cut]
            outs = pool.push(ids, wavs, vids)
            for s, n, k in zip(ids, na, nf):
                pos[s][0] += n
                pos[s][1] += k
        assert len(outs) == len(ids)
        if y_of is not None and want["rows"]:
            hist = {s: (xs[s][:pos[s][0]], vs[s][:, :, :pos[s][1]]) for s in ids}
            exw, evw = SO.frame_rows(want["rows"], hist, {s: tuple(pos[s]) for s in ids}, window, hop, K)
            assert np.array_equal(seen["xw"], exw), f"audio windows differ in {kind} {ids} {na} {nf} at {counters}"
            assert np.array_equal(seen["vw"], evw), f"video windows differ in {kind} {ids} {na} {nf} at {counters}"
            for i, (s, n) in enumerate(want["rows"]):
                olas[s].feed(n, seen["y"][i])
                y_max[s] = max(y_max[s], float(np.abs(seen["y"][i]).max()))
        for r, (s, out) in enumerate(zip(ids, outs)):
            o, end = want["ranges"][r]
            assert tuple(out.shape) == (K, end - o), (kind, ids, r)
            res = host(out)
            got[s].append(res)
            if end > o:
                assert out.data_ptr() % 128 == 0, (kind, ids, r)  # every slot's block starts on a 128-byte line
            if y_of is not None and end > o:
                ref = olas[s].take(o, end)
                err, bound = float(np.abs(res - ref).max()), ola_bound(window, hop, np.float64(y_max[s]))
                assert np.isfinite(res).all() and err <= bound, (kind, ids, s, err, bound)
                worst = max(worst, err / bound)
                if hop == window:
                    assert np.array_equal(res, ref.astype(np.float32)), (kind, ids, s)
            assert pool.counters(s) == want["new"][s]
        counters = want["new"]
    return {s: np.concatenate(g, axis=1) for s, g in got.items()}, worst


def synthetic(xw, vw, K):
    """Row-wise, depends on the audio window, on the target's own lips and on k."""
    rows = xw.shape[0]
    gain = (1.0 + 0.5 * np.tanh(vw.mean(axis=(1, 2)))).reshape(rows, K) * (1.0 + np.arange(K))
    return np.tanh(xw)[:, None, :] * gain[:, :, None]


def three_slots(window, hop, max_chunk, K, seed):
    rng = np.random.RandomState(seed)
    C = VO.capacity(window, max_chunk)
    Ls = [2 * C + hop + 1, window + 3 * hop - 1, window - 1]  # slot 0 wraps its rings twice; slot 2 is one short window
    Tvs = [-(-Ls[0] // SPF), -(-Ls[1] // SPF) - 2, -(-Ls[2] // SPF)]  # slot 1 is two frames short at its flush
    xs = {s: rng.randn(L).astype(np.float32) for s, L in enumerate(Ls)}
    vs = {s: rng.randn(K, 512, Tv).astype(np.float32) for s, Tv in enumerate(Tvs)}
    sizes = VO.chunk_sizes(hop, max_chunk)  # 0 among them: empty pushes on either side
    sch = {s: VO.schedule(Ls[s], Tvs[s], sizes, MODES[s], window, hop, max_chunk, start=3 * s + 1) for s in range(3)}
    return xs, vs, VO.events(sch)


# ---------------------------------------------------------------- 1 + 2. the launches on synthetic windows
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("window,hop", PLANS)
def test_ingest_framing_is_a_copy_and_overlap_add_meets_the_oracle(window, hop, K):
    xs, vs, events = three_slots(window, hop, window, K, window + hop + K)
    assert any(0 in na for kind, _, na, _ in events if kind == "push") and any(0 in nf for kind, _, _, nf in events if kind == "push")
    res = []
    for stacked in (False, True):
        pool = open_pool(K, slots=3, window=window, hop=hop, max_batch=2)
        got, worst = drive(pool, xs, vs, events, window, hop, window, y_of=synthetic, stacked=stacked)
        for s in xs:
            assert got[s].shape == (K, xs[s].shape[0])
        res.append(got)
    for s in xs:
        assert np.array_equal(res[0][s], res[1][s]), f"K allocations and one (K,512,m) tensor differ at slot {s}"
    print(f"[live speakers] window {window} hop {hop} K {K}: {len(events)} ticks, worst overlap-add error {worst:.3f} of the bound")


@pytest.mark.parametrize("window,hop", PLANS)
def test_longform_framing_kernel_is_bit_exact(window, hop):
    L_, B, K = lib(), 2, 3
    L = window + 3 * hop - 1
    Tv = -(-L // SPF) - 2
    rng = np.random.RandomState(window + hop)
    x, v = rng.randn(B, L).astype(np.float32), rng.randn(B, K, 512, Tv).astype(np.float32)
    exw, evw = SO.frame_long(x, v, window, hop)
    N = exw.shape[0] // B
    xd, vd = offset_view(x), dev(v)  # the recording 4 bytes into its allocation: dword loads
    xw = L_.empty(B * N, window, device=xd.device)
    vw = L_.empty(B * N * K, 512, window // SPF, device=xd.device)
    L_.check(L_.load().rtfs_longform_frame_speakers_f32(L_.ptr(xd), L_.ptr(vd), L_.ptr(xw), L_.ptr(vw), B, K, L, Tv, window, hop,
                                                        L_.stream_of(xd)), "rtfs_longform_frame_speakers_f32")
    assert np.array_equal(host(xw), exw) and np.array_equal(host(vw), evw)
    # one track through the single-track entry: K = 1 of the same kernel, == track 0 of the K = 3 rows
    v0 = np.ascontiguousarray(v[:, 0])
    xw1 = L_.empty(B * N, window, device=xd.device)
    vw1 = L_.empty(B * N, 512, window // SPF, device=xd.device)
    L_.check(L_.load().rtfs_longform_frame_f32(L_.ptr(xd), L_.ptr(dev(v0)), L_.ptr(xw1), L_.ptr(vw1), B, L, Tv, window, hop,
                                               L_.stream_of(xd)), "rtfs_longform_frame_f32")
    exw1, evw1 = SO.frame_long(x, v[:, :1], window, hop)
    assert np.array_equal(host(xw1), exw) and np.array_equal(host(vw1), host(vw)[0::K])
    assert np.array_equal(host(xw1), exw1) and np.array_equal(host(vw1), evw1)
    for bad in (0, 17):
        assert L_.load().rtfs_longform_frame_speakers_f32(L_.ptr(xd), L_.ptr(vd), L_.ptr(xw), L_.ptr(vw), B, bad, L, Tv, window, hop,
                                                          L_.stream_of(xd)) == -4


# ---------------------------------------------------------------- 3. composition with the real separator
def faces(L, K, seed):
    """One mixture (L,) and K lip tracks (K,512,ceil(L/640))."""
    Tv = -(-L // SPF)
    w = make_inputs(1, L, Tv, seed)[0][0]
    return w, np.stack([make_inputs(1, L, Tv, seed + 100 * (k + 1))[1][0] for k in range(K)])


@pytest.mark.parametrize("hop", [2560, 1920])
def test_streams_equal_separate_long_of_every_face(hop):
    m, K = model(4), 2
    window, max_chunk, max_batch = 5120, 5120, 4
    Ls = [12000, 5120, 17283]
    xs, vs = {}, {}
    for s, L in enumerate(Ls):
        xs[s], vs[s] = faces(L, K, 80 + s)
    sizes = [1, 2561, 639, 0, 5120, 640, 1919, 3000]
    sch = {s: VO.schedule(Ls[s], vs[s].shape[2], sizes, MODES[s], window, hop, max_chunk, start=2 * s) for s in range(3)}
    events = VO.events(sch)
    pool = m.open_streams(3, window=window, hop=hop, max_chunk=max_chunk, max_batch=max_batch, speakers=K)
    got, _ = drive(pool, xs, vs, events, window, hop, max_chunk)
    # separate_speakers on exactly the chunks the oracle's schedule lists: every tick's rows in chunks of max_batch // K windows
    step, Wv = max(1, max_batch // K), window // SPF
    counters, pos = {s: (0, 0, 0, 0) for s in xs}, {s: [0, 0] for s in xs}
    olas, ref = {s: SO.OverlapAdd(window, hop, K) for s in xs}, {s: [] for s in xs}
    y_max = 0.0
    for kind, ids, na, nf in events:
        want = SO.tick(counters, ids, na, nf, window, hop, max_chunk, K, kind == "flush")
        if kind == "push":
            for s, n, k in zip(ids, na, nf):
                pos[s][0] += n
                pos[s][1] += k
        if want["rows"]:
            hist = {s: (xs[s][:pos[s][0]], vs[s][:, :, :pos[s][1]]) for s in ids}
            xw, vw = SO.frame_rows(want["rows"], hist, {s: tuple(pos[s]) for s in ids}, window, hop, K)
            vw = vw.reshape(len(want["rows"]), K, 512, Wv)
            y = np.concatenate([host(m.separate_speakers(dev(xw[c:c + step]), dev(vw[c:c + step]))) for c in range(0, len(want["rows"]), step)])
            y_max = max(y_max, float(np.abs(y).max()))
            for i, (s, n) in enumerate(want["rows"]):
                olas[s].feed(n, y[i])
        for s, (o, end) in zip(ids, want["ranges"]):
            ref[s].append(olas[s].take(o, end))
        counters = want["new"]
    for s, L in enumerate(Ls):
        want = np.concatenate(ref[s], axis=1)
        err, bound = float(np.abs(got[s] - want).max()), ola_bound(window, hop, np.float64(y_max))
        print(f"[live speakers] hop {hop} slot {s} L {L}: vs oracle overlap-add of separate_speakers on the tick chunks {err:.3e} (bound {bound:.3e})")
        assert got[s].shape == (K, L) and np.isfinite(got[s]).all()
        es = []
        for k in range(K):
            whole = host(m.separate_long(dev(xs[s][None]), dev(vs[s][k][None]), window=window, hop=hop))[0, 0]
            es.append(rel_err(got[s][k], whole))
        print(f"[live speakers] hop {hop} slot {s} L {L}: vs separate_long(whole, lips k) max-rel {[f'{e:.3e}' for e in es]}")
        assert err <= bound, (s, err, bound)
        assert max(es) <= 1e-4, (s, es)


@pytest.mark.parametrize("B,K", [(1, 1), (1, 2), (2, 3)])
@pytest.mark.parametrize("hop", [2560, 1920])
def test_separate_long_speakers_equals_separate_long_per_track(hop, B, K):
    m, window, L = model(4), 5120, 12000
    Tv = -(-L // SPF) - (2 if B == 2 else 0)
    x = np.stack([faces(L, 1, 60 + b)[0] for b in range(B)])
    v = np.stack([faces(L, K, 70 + b)[1][:, :, :Tv] for b in range(B)])
    got = host(m.separate_long_speakers(dev(x), dev(v), window=window, hop=hop, max_batch=4))
    assert got.shape == (B, K, L) and np.isfinite(got).all()
    for k in range(K):
        want = host(m.separate_long(dev(x), dev(np.ascontiguousarray(v[:, k])), window=window, hop=hop, max_batch=4))[:, 0]
        e = rel_err(got[:, k], want)
        print(f"[long speakers] hop {hop} B {B} K {K} track {k}: max-rel vs separate_long {e:.3e}")
        assert e <= 1e-4, (k, e)


# ---------------------------------------------------------------- 4. camera
def test_camera_streams_equal_separate_recording_of_every_face():
    import rtfs_net_amd as R
    from tests.test_hip_live_video import rois
    from tests.test_hip_many import video_model
    window, hop, mc, K = 5120, 2560, 5120, 2
    system = R.System(audio_model=model(4), video_model=video_model())
    Ls = [2 * window + hop + 7, window - 1]
    rng = np.random.RandomState(5)
    wavs, tracks, sch = {}, {}, {}
    for s, L in enumerate(Ls):
        Tv = -(-L // SPF) - (2 if s == 1 else 0)
        wavs[s] = (0.1 * rng.randn(L)).astype(np.float32)
        tracks[s] = np.stack([rois(Tv, 96, 96, 40 + 10 * s + k) for k in range(K)])
        sch[s] = LV.camera_schedule(L, Tv, VO.chunk_sizes(hop, mc), ("lag", "lead")[s], window, hop, mc, mc + LV.SLACK, start=s + 1)
    pool = system.open_camera_streams(2, window=window, hop=hop, speakers=K, roi_hw=(96, 96), max_batch=4)
    assert type(pool) is R.SpeakerCameraStreamPool and pool.lips.slots == 2 * K
    embs = {t: [] for t in range(2 * K)}
    lip_tick = pool.lips._tick

    def recording_tick(ids, *a, **kw):
        outs = lip_tick(ids, *a, **kw)
        for t, o in zip(ids, outs):
            embs[t].append(host(o).copy())
        return outs

    pool.lips._tick = recording_tick
    pos, got = {s: [0, 0] for s in wavs}, {s: [] for s in wavs}
    for i in range(max(len(v) for v in sch.values()) + 1):
        done = [s for s, v in sch.items() if len(v) == i]
        if done:
            for s, o in zip(done, pool.flush(done)):
                got[s].append(host(o))
        ids = [s for s, v in sch.items() if len(v) > i]
        if ids:
            na, nf = [sch[s][i][0] for s in ids], [sch[s][i][1] for s in ids]
            outs = pool.push(ids, [dev(wavs[s][pos[s][0]:pos[s][0] + a]) for s, a in zip(ids, na)],
                             [dev(tracks[s][:, pos[s][1]:pos[s][1] + f]) for s, f in zip(ids, nf)])
            for s, a, f, o in zip(ids, na, nf, outs):
                pos[s][0] += a
                pos[s][1] += f
                got[s].append(host(o))
    vm = video_model()
    for s, L in enumerate(Ls):
        res = np.concatenate(got[s], axis=1)
        assert res.shape == (K, L) and np.isfinite(res).all() and pool.counters(s) == ((0, 0, 0, 0), (0, 0))
        for k in range(K):
            ref = host(system.separate_recording(dev(wavs[s]), 16000, dev(tracks[s][k]), window=window, hop=hop))[0, 0]
            e = rel_err(res[k], ref)
            with torch.no_grad():
                whole = host(vm(dev(LV.prepare_u8(tracks[s][k]))[None, None]))[0]
            emb = np.concatenate(embs[s * K + k], axis=1)
            same = emb.shape == whole.shape and np.array_equal(emb, whole)
            print(f"[camera speakers] slot {s} face {k} L {L}: rel_err vs separate_recording {e:.3e}; embeddings bit-equal to the whole track: "
                  f"{same} (max abs diff {float(np.abs(emb - whole).max()) if emb.shape == whole.shape else -1:.3e})")
            assert e <= 1e-4, (s, k, e)
            assert same, (s, k)


# ---------------------------------------------------------------- 5. slot reuse
def stream_once(pool, slot, x, v, sizes, window, hop):
    out, a, f = [], 0, 0
    for na, nf in VO.schedule(x.shape[0], v.shape[2], sizes, "step", window, hop, window):
        out.append(host(pool.push([slot], [dev(x[a:a + na])], [dev(np.ascontiguousarray(v[:, :, f:f + nf]))])[0]))
        a, f = a + na, f + nf
    out.append(host(pool.flush([slot])[0]))
    return np.concatenate(out, axis=1)


def test_a_slot_is_clean_after_flush_and_after_reset():
    m, window, hop, K = model(4), 5120, 2560, 2
    (w1, e1), (w2, e2) = faces(9000, K, 91), faces(13001, K, 92)
    sizes = [2000, 640, 3333]
    fresh = stream_once(m.open_streams(2, window=window, hop=hop, speakers=K), 1, w2, e2, sizes, window, hop)
    pool = m.open_streams(2, window=window, hop=hop, speakers=K)
    stream_once(pool, 1, w1, e1, sizes, window, hop)
    assert np.array_equal(stream_once(pool, 1, w2, e2, sizes, window, hop), fresh)  # after a flush
    pool.push([1], [dev(w1[:4000])], [dev(np.ascontiguousarray(e1[:, :, :6]))])  # a stream dropped half way, sums pending
    pool.push([1], [dev(w1[4000:7000])], [dev(np.ascontiguousarray(e1[:, :, 6:11]))])
    assert pool.counters(1)[2] == 1
    pool.reset([1])
    assert pool.counters(1) == (0, 0, 0, 0)
    assert np.array_equal(stream_once(pool, 1, w2, e2, sizes, window, hop), fresh)  # after a reset
    assert fresh.shape == (K, 13001) and np.isfinite(fresh).all()


# ---------------------------------------------------------------- 6. refusals on device tensors
def test_refusals_launch_nothing_and_leave_no_trace():
    m, window, hop, K = model(4), 5120, 2560, 2
    w, e = faces(12000, K, 93)
    x, v = dev(w), dev(e)
    pushes = [(0, 3000, 0, 0), (3000, 6000, 0, 4), (6000, 10000, 4, 12), (10000, 12000, 12, 19)]  # the video lags, then catches up
    cut = lambda f0, f1: v[:, :, f0:f1].contiguous()  # noqa: E731
    none, one = cut(0, 0), cut(0, 1)

    def run(with_refusals):
        pool, out = m.open_streams(2, window=window, hop=hop, speakers=K), []
        for a0, a1, f0, f1 in pushes:
            if with_refusals:
                count, before = lib().load().rtfs_debug_launch_count(), [pool.counters(s) for s in range(2)]
                bad = [([2], [x[:10]], [none]), ([0, 0], [x[:10]] * 2, [one] * 2), ([1, 0], [x[:10], x[:5121]], [one, one]),
                       ([0], [x[:10].cpu()], [one]), ([0], [x[:10].double()], [one]), ([0], [x[:10]], [v[:, :500, :1].contiguous()]),
                       ([0], [x[:10]], [[one[0], cut(0, 2)[1]]]), ([0], [x[:10]], [[one[0]]]), ([0], [x[:10]], [cut(0, 1)[0]]),
                       ([0], [x[:10]], [torch.cat([one, one, one])]), ([0], [x[:10]], [[one[0], one[1].cpu()]])]
                if a0 == 6000:  # 6000 samples, 4 frames, no window yet: 6000 + 5000 > 10240 would overwrite what window 0 needs
                    bad.append(([1, 0], [x[:10], x[:5000]], [one, none]))
                for ids, wavs, vids in bad:
                    with pytest.raises(ValueError):
                        pool.push(ids, wavs, vids)
                with pytest.raises(ValueError):
                    pool.flush([0, 5])
                with pytest.raises(ValueError):
                    m.open_streams(2, window=window, hop=hop, speakers=17)
                with pytest.raises(ValueError):
                    m.separate_long_speakers(x, v[None, :, :256], window=window, hop=hop)
                assert lib().load().rtfs_debug_launch_count() == count and [pool.counters(s) for s in range(2)] == before
            out.append(host(pool.push([0], [x[a0:a1]], [cut(f0, f1)])[0]))
        out.append(host(pool.flush([0])[0]))
        return np.concatenate(out, axis=1)

    clean = run(False)
    assert np.array_equal(run(True), clean) and clean.shape == (K, 12000)


# ---------------------------------------------------------------- 7. poisoned memory
CASES = "test_ingest or test_longform_framing or test_streams_equal or test_separate_long or test_camera or test_a_slot or test_refusals"
ABNORMAL = (124, 134, 137, 139)


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
def test_poisoned():
    """This file's cases in a fresh child process per pattern, with every workspace / output / state buffer poisoned
    (tests/test_hip_live.py's discipline: a time limit per child, and no second child after an abnormal exit)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pattern in ("nan", "big"):
        env = dict(os.environ, RTFS_POISON_WS=pattern)
        try:
            pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_live_speakers.py"), "-m", "gpu", "-q", "-p",
                                 "no:cacheprovider", "-k", CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s; no further child started")
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            pytest.fail(f"RTFS_POISON_WS={pattern}: abnormal exit status {pr.returncode}; no further child started\n{pr.stdout[-3000:]}")
        assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
