"""Live streams whose faces come and go (AVNet.open_streams(max_speakers=Kmax) / FaceStreamPool, System.open_camera_streams(
max_speakers=Kmax), rtfs_live_ingest_frame_faces_f32, rtfs_live_overlap_add_faces_f32) against tests/live_faces_oracle.py:

1. framing is a copy and the overlap-add meets the float64 oracle of every face (test_hip_longform.ola_bound, hop == window bit-equal),
   over the plans of tests/test_hip_live.py with a schedule that holds every case the kernels tell apart (asserted, see
   ``required_scripts``), chunk tensors 4 bytes into their allocations, the tracks once as separate allocations and once stacked;
2. composition with the real separator: every face == separate_long of the stream cut at its birth (tests/util.rel_err <= 1e-4), a
   dropped face == the leading part of that;
3. == the oracle overlap-add of separate_speakers(counts=) on exactly the chunks the schedule lists (ola_bound);
4. all planes from the first push: bit-equal to SpeakerStreamPool(K = Kmax) on the same pushes;
5. the camera pool against System.separate_recording per face, lip embeddings bit-equal to video_model on the whole track;
6. slot reuse after flush and after reset, bit-equal to a fresh pool, faces cleared;
7. refusals on device tensors launch nothing and leave no trace;
8. the cases again in child processes on poisoned memory (RTFS_POISON_WS = nan, big)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.params import make_inputs
from tests import live_faces_oracle as FO
from tests import live_oracle as VO
from tests import test_hip_live_speakers as SS
from tests.test_hip_live import MODES, PLANS, Sized, offset_view
from tests.test_hip_longform import dev, host, lib, model, ola_bound
from tests.test_live_faces_host import Runner
from tests.util import rel_err

pytestmark = pytest.mark.gpu

SPF = 640
POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")


def open_pool(Kmax, **kw):
    from rtfs_net_amd import streaming
    return streaming.open_face_streams(Sized(model(4), 1), max_speakers=Kmax, **kw)


def synthetic(xw, vw, js):
    """Row-wise: a target's value depends on its audio window, on its own lips and on its face id."""
    return np.tanh(xw) * ((1.0 + 0.5 * np.tanh(vw.mean(axis=(1, 2)))) * (1.0 + js))[:, None]


def pushes_of(c, steps, window, hop, max_chunk):
    for _, na, nf in steps:
        c = VO.push_one(c, na, nf, window, hop, max_chunk)[0]
    return c


def required_scripts(window, hop, max_chunk):
    """Three slots, Kmax = 3.  Slot 0: three faces from the start, rings wrapped twice, face 1 dropped in mid-stream and a new face
    later added on the same plane.  Slot 1: a second face joins at f = 1 (off a hop boundary when hop > 640) while window 0 still waits
    for audio, then one audio chunk makes the windows on both sides of its birth ready at once (window > hop); two frames short at the
    flush, in front of which a third face joins and receives nothing.  Slot 2: one short window with two faces."""
    W, H, Wv, Hv = window, hop, window // SPF, hop // SPF
    C = VO.capacity(W, max_chunk)
    sizes = VO.chunk_sizes(H, max_chunk)
    L0 = 2 * C + H + 1
    s0 = [("push",) + p for p in VO.schedule(L0, -(-L0 // SPF), sizes, "step", W, H, max_chunk, start=1)]
    i1, i2 = len(s0) // 3, 2 * len(s0) // 3
    s0 = [("add", None)] * 3 + s0[:i1] + [("drop", 1)] + s0[i1:i2] + [("add", None)] + s0[i2:]
    head = [("push", W - 1, 1), ("add", None), ("push", 0, Wv), ("push", 0, Hv - 1), ("push", W, 0)]
    L1 = 2 * W - 1 + 2 * H + 3
    rest = FO.continue_schedule(pushes_of((0, 0, 0, 0), [h for h in head if h[0] == "push"], W, H, max_chunk), L1, -(-L1 // SPF) - 2, sizes,
                                W, H, max_chunk, start=4)
    s1 = [("add", None)] + head + [("push",) + p for p in rest] + [("add", None)]
    L2 = W - 1
    s2 = [("add", None)] * 2 + [("push",) + p for p in VO.schedule(L2, -(-L2 // SPF), sizes, "lead", W, H, max_chunk, start=7)]
    return {0: s0, 1: s1, 2: s2}, (L0, L1, L2)


# ---------------------------------------------------------------- 1. the launches on synthetic windows
@pytest.mark.parametrize("window,hop", PLANS)
def test_framing_is_a_copy_and_overlap_add_meets_the_oracle(window, hop):
    scripts, Ls = required_scripts(window, hop, window)
    events = FO.merge(scripts)
    res = []
    for stacked in (False, True):
        pool = open_pool(3, slots=3, window=window, hop=hop, max_batch=2)
        run = Runner(pool, 3, 3, window, hop, window, window + hop, offset_view, host, stacked=stacked, y_of=synthetic, bound=ola_bound).run(events)
        seen = run.seen
        assert seen["three_from_start"] >= {0} and seen["wraps"][0] >= 2, seen
        assert seen["reused_plane_stale"] >= 1 and seen["no_frame_face"] >= 1 and seen["empty_audio"] and seen["empty_video"], seen
        assert (seen["join_off_hop_pending"] >= 1) == (hop > SPF), seen  # at hop = 640 every frame count is a hop boundary
        assert (seen["both_sides"] >= 1 and seen["ragged"] >= 1) == (window > hop), seen  # at hop == window a tick of <= window samples emits one window
        by_slot = {s: [r for r in run.closed if r["s"] == s] for s in range(3)}
        assert [len(by_slot[s]) for s in range(3)] == [4, 3, 2]
        short = by_slot[1][0]
        assert short["c_end"][1] == -(-Ls[1] // SPF) - 2 and short["c_end"][0] == Ls[1]  # two frames short at its flush
        assert all(sum(g.shape[0] for g in r["got"]) == Ls[2] for r in by_slot[2]) and Ls[2] < window
        for r in run.closed:
            n = sum(g.shape[0] for g in r["got"])
            if r["state"] == "flushed":
                assert n == r["c_end"][0] - r["b"] * hop, (r["s"], r["j"], n)
            elif r["state"] == "idle":
                assert n == 0
        res.append([np.concatenate(r["got"]) if r["got"] else np.zeros(0) for r in run.closed])
    assert all(np.array_equal(a, b) for a, b in zip(*res)), "separate allocations and one stacked tensor differ"
    print(f"[live faces] window {window} hop {hop}: {run.ticks} ticks, worst overlap-add error {run.worst:.3f} of the bound; seen {seen}")


# ---------------------------------------------------------------- 2 + 3. composition with the real separator
def chunks_of(counts, max_batch):
    """The chunking rule: consecutive windows whose targets total at most max_batch; a window with more goes alone."""
    out, w0, t0, t = [], 0, 0, 0
    for w, c in enumerate(counts):
        if w > w0 and t - t0 + c > max_batch:
            out.append((w0, w, t0, t))
            w0, t0 = w, t
        t += c
    return out + ([(w0, len(counts), t0, t)] if len(counts) > w0 else [])


def after_windows(steps, k, window, hop, max_chunk):
    """The number of leading pushes of ``steps`` after which k windows have been emitted."""
    c = (0, 0, 0, 0)
    for i, (_, na, nf) in enumerate(steps):
        if c[2] >= k:
            return i
        c = VO.push_one(c, na, nf, window, hop, max_chunk)[0]
    raise AssertionError("the schedule never emits that many windows before its flush")


@pytest.mark.parametrize("hop", [2560, 1920])
def test_streams_equal_separate_long_from_the_birth_of_every_face(hop):
    m = model(4)
    window, max_chunk, max_batch, Kmax = 5120, 5120, 4, 3
    Ls = [12000, 17283, 14000]
    wav = {s: make_inputs(1, L, -(-L // SPF), 80 + s)[0][0] for s, L in enumerate(Ls)}
    lips = {(s, j): make_inputs(1, L, -(-L // SPF), 80 + s + 100 * (j + 1))[1][0] for s, L in enumerate(Ls) for j in range(Kmax)}
    draw = (lambda s, a0, n: wav[s][a0:a0 + n], lambda s, j, f0, k: np.ascontiguousarray(lips[s, j][:, f0:f0 + k]))
    sizes = [1, 2561, 639, 0, 5120, 640, 1919, 3000]
    sch = {s: [("push",) + p for p in VO.schedule(Ls[s], -(-Ls[s] // SPF), sizes, MODES[s], window, hop, max_chunk, start=2 * s)] for s in range(3)}
    i1, i2 = after_windows(sch[1], 2, window, hop, max_chunk), after_windows(sch[2], 1, window, hop, max_chunk)
    scripts = {0: [("add", None)] + sch[0],  # one face
               1: [("add", None)] * 3 + sch[1][:i1] + [("drop", 1)] + sch[1][i1:],  # three faces, one leaves after two windows
               2: [("add", None)] + sch[2][:i2] + [("add", None)] + sch[2][i2:]}  # one face, a second joins after the first window
    pool = m.open_streams(3, window=window, hop=hop, max_chunk=max_chunk, max_batch=max_batch, max_speakers=Kmax)

    def sep(xw, vw, row_counts):
        live = [w for w, c in enumerate(row_counts) if c]
        counts = [row_counts[w] for w in live]
        return np.concatenate([host(m.separate_speakers(dev(xw[live][w0:w1]), dev(vw[t0:t1]), counts=counts[w0:w1]))
                               for w0, w1, t0, t1 in chunks_of(counts, max_batch)])

    run = Runner(pool, 3, Kmax, window, hop, max_chunk, 0, offset_view, host, sep=sep, bound=ola_bound, draw=draw).run(FO.merge(scripts))
    print(f"[live faces] hop {hop}: vs oracle overlap-add of separate_speakers(counts=) on the tick chunks, worst {run.worst:.3f} of ola_bound")
    states = sorted((r["s"], r["state"]) for r in run.closed)
    assert states == [(0, "flushed"), (1, "dropped"), (1, "flushed"), (1, "flushed"), (2, "flushed"), (2, "flushed")], states
    assert any(r["b"] > 0 for r in run.closed if r["s"] == 2)
    for r in run.closed:
        got = np.concatenate(r["got"])
        b, (a, f) = r["b"], r["c_end"][:2]
        whole = host(m.separate_long(dev(r["x"][None, b * hop:a]), dev(np.ascontiguousarray(r["v"][None, :, b * hop // SPF:f])), window=window,
                                     hop=hop))[0, 0]
        assert got.shape[0] == (whole.shape[0] if r["state"] == "flushed" else r["c_end"][3] - b * hop) and got.shape[0] > 0
        e = rel_err(got, whole[:got.shape[0]])
        print(f"[live faces] hop {hop} slot {r['s']} face {r['j']} born {b} {r['state']}: {got.shape[0]} samples, rel_err vs separate_long from the birth {e:.3e}")
        assert np.isfinite(got).all() and e <= 1e-4, (r["s"], r["j"], e)


# ---------------------------------------------------------------- 4. all planes from the start
@pytest.mark.parametrize("window,hop", PLANS)
def test_all_planes_from_the_start_is_the_speaker_pool_bit_for_bit(window, hop):
    K = 3
    xs, vs, events = SS.three_slots(window, hop, window, K, window + hop + K)
    want, _ = SS.drive(SS.open_pool(K, slots=3, window=window, hop=hop, max_batch=2), xs, vs, events, window, hop, window, y_of=SS.synthetic)
    pool = open_pool(K, slots=3, window=window, hop=hop, max_batch=2)

    def fake(row_counts):
        rows = len(row_counts)
        assert list(row_counts) == [K] * rows
        y = SS.synthetic(host(pool._xw[:rows]), host(pool._vw[:rows * K]), K).astype(np.float32)
        pool._yt[:rows * K].copy_(dev(y.reshape(rows * K, window)))

    pool._forward_targets = fake
    got, pos = {s: {k: [] for k in range(K)} for s in xs}, {s: [0, 0] for s in xs}
    for s in xs:
        assert [pool.add_face(s) for _ in range(K)] == list(range(K))
    for kind, ids, na, nf in events:
        if kind == "flush":
            outs = pool.flush(ids)
        else:
            outs = pool.push(ids, [offset_view(xs[s][pos[s][0]:pos[s][0] + n]) for s, n in zip(ids, na)],
                             [offset_view(np.ascontiguousarray(vs[s][:, :, pos[s][1]:pos[s][1] + n])) for s, n in zip(ids, nf)])
            for s, n, k in zip(ids, na, nf):
                pos[s][0] += n
                pos[s][1] += k
        for s, out in zip(ids, outs):
            for k in range(K):
                got[s][k].append(host(out[k]))
    for s in xs:
        res = np.stack([np.concatenate(got[s][k]) for k in range(K)])
        assert res.shape == want[s].shape and np.array_equal(res, want[s]), (s, float(np.abs(res - want[s]).max()))


# ---------------------------------------------------------------- 5. camera
def test_camera_streams_equal_separate_recording_of_every_face():
    import rtfs_net_amd as R
    from tests import live_video_oracle as LV
    from tests.test_hip_live_video import rois
    from tests.test_hip_many import video_model
    window, hop, mc, Kmax = 5120, 2560, 5120, 2
    system = R.System(audio_model=model(4), video_model=video_model())
    Ls, Ks = [2 * window + hop + 7, window - 1], [2, 1]
    rng = np.random.RandomState(5)
    wavs, tracks, sch = {}, {}, {}
    for s, L in enumerate(Ls):
        Tv = -(-L // SPF) - (2 if s == 1 else 0)
        wavs[s] = (0.1 * rng.randn(L)).astype(np.float32)
        tracks[s] = np.stack([rois(Tv, 96, 96, 40 + 10 * s + k) for k in range(Ks[s])])
        sch[s] = LV.camera_schedule(L, Tv, VO.chunk_sizes(hop, mc), ("lag", "lead")[s], window, hop, mc, mc + LV.SLACK, start=s + 1)
    pool = system.open_camera_streams(2, window=window, hop=hop, max_speakers=Kmax, roi_hw=(96, 96), max_batch=4)
    assert type(pool) is R.FaceCameraStreamPool and pool.lips.slots == 2 * Kmax and type(pool.audio) is R.FaceStreamPool
    for kw in (dict(max_speakers=2, speakers=2), dict(max_speakers=17), dict(max_speakers=2, sample_rate=48000)):
        with pytest.raises(ValueError):
            system.open_camera_streams(2, window=window, hop=hop, **kw)
    assert [pool.add_face(0), pool.add_face(0), pool.add_face(1, 1)] == [0, 1, 1]  # slot 1's face sits on plane 1: lip track 3
    plane = {0: [0, 1], 1: [1]}
    embs = {t: [] for t in range(2 * Kmax)}
    lip_tick = pool.lips._tick

    def recording_tick(ids, *a, **kw):
        outs = lip_tick(ids, *a, **kw)
        for t, o in zip(ids, outs):
            embs[t].append(host(o).copy())
        return outs

    pool.lips._tick = recording_tick
    pos, got = {s: [0, 0] for s in wavs}, {s: {j: [] for j in plane[s]} for s in wavs}
    joined = False
    for i in range(max(len(v) for v in sch.values()) + 1):
        done = [s for s, v in sch.items() if len(v) == i]
        if done:
            for s, o in zip(done, pool.flush(done)):
                for j in plane[s]:
                    got[s][j].append(host(o[j]))
        ids = [s for s, v in sch.items() if len(v) > i]
        if ids:
            na, nf = [sch[s][i][0] for s in ids], [sch[s][i][1] for s in ids]
            outs = pool.push(ids, [dev(wavs[s][pos[s][0]:pos[s][0] + a]) for s, a in zip(ids, na)],
                             [dev(tracks[s][:, pos[s][1]:pos[s][1] + f]) for s, f in zip(ids, nf)])
            for s, a, f, o in zip(ids, na, nf, outs):
                pos[s][0] += a
                pos[s][1] += f
                for j in plane[s]:
                    got[s][j].append(host(o[j]))
            if 1 in ids and not joined and any(pool.counters(1)[0]):
                before = (pool.counters(1), pool.faces(1))
                with pytest.raises(ValueError, match="idle"):
                    pool.add_face(1)  # a face joins a camera stream on an idle slot only
                assert (pool.counters(1), pool.faces(1)) == before
                joined = True
    assert joined
    vm = video_model()
    for s, L in enumerate(Ls):
        assert pool.counters(s) == ((0, 0, 0, 0), (0, 0)) and pool.faces(s) == []
        for k, j in enumerate(plane[s]):
            res = np.concatenate(got[s][j])
            assert res.shape == (L,) and np.isfinite(res).all()
            ref = host(system.separate_recording(dev(wavs[s]), 16000, dev(tracks[s][k]), window=window, hop=hop))[0, 0]
            e = rel_err(res, ref)
            with torch.no_grad():
                whole = host(vm(dev(LV.prepare_u8(tracks[s][k]))[None, None]))[0]
            emb = np.concatenate(embs[s * Kmax + j], axis=1)
            same = emb.shape == whole.shape and np.array_equal(emb, whole)
            print(f"[camera faces] slot {s} face {j} L {L}: rel_err vs separate_recording {e:.3e}; embeddings bit-equal to the whole track: {same}")
            assert e <= 1e-4, (s, j, e)
            assert same, (s, j)


# ---------------------------------------------------------------- 6. slot reuse
def faces(L, K, seed):
    Tv = -(-L // SPF)
    return make_inputs(1, L, Tv, seed)[0][0], np.stack([make_inputs(1, L, Tv, seed + 100 * (k + 1))[1][0] for k in range(K)])


def stream_once(pool, slot, x, v, sizes, window, hop):
    K = v.shape[0]
    assert pool.faces(slot) == [] and [pool.add_face(slot) for _ in range(K)] == list(range(K))
    out, a, f = [], 0, 0
    for na, nf in VO.schedule(x.shape[0], v.shape[2], sizes, "step", window, hop, window):
        res = pool.push([slot], [dev(x[a:a + na])], [dev(np.ascontiguousarray(v[:, :, f:f + nf]))])[0]
        out.append(np.stack([host(res[k]) for k in range(K)]))
        a, f = a + na, f + nf
    res = pool.flush([slot])[0]
    out.append(np.stack([host(res[k]) for k in range(K)]))
    assert pool.faces(slot) == []
    return np.concatenate(out, axis=1)


def test_a_slot_is_clean_after_flush_and_after_reset():
    m, window, hop, K = model(4), 5120, 2560, 2
    (w1, e1), (w2, e2) = faces(9000, K, 91), faces(13001, K, 92)
    sizes = [2000, 640, 3333]
    fresh = stream_once(m.open_streams(2, window=window, hop=hop, max_speakers=3), 1, w2, e2, sizes, window, hop)
    pool = m.open_streams(2, window=window, hop=hop, max_speakers=3)
    stream_once(pool, 1, w1, e1, sizes, window, hop)
    assert np.array_equal(stream_once(pool, 1, w2, e2, sizes, window, hop), fresh)  # after a flush
    assert pool.add_face(1, 2) == 2 and pool.add_face(1, 0) == 0  # other planes than the fresh pool's, sums pending at the reset
    pool.push([1], [dev(w1[:4000])], [dev(np.ascontiguousarray(e1[:, :, :6]))])
    pool.push([1], [dev(w1[4000:7000])], [dev(np.ascontiguousarray(e1[:, :, 6:11]))])
    assert pool.counters(1)[2] == 1 and pool.faces(1) == [0, 2]
    pool.reset([1])
    assert pool.counters(1) == (0, 0, 0, 0) and pool.faces(1) == []
    assert np.array_equal(stream_once(pool, 1, w2, e2, sizes, window, hop), fresh)  # after a reset
    assert fresh.shape == (K, 13001) and np.isfinite(fresh).all()


# ---------------------------------------------------------------- 7. refusals on device tensors
def test_refusals_launch_nothing_and_leave_no_trace():
    m, window, hop = model(4), 5120, 2560
    w, e = faces(12000, 2, 93)
    x, v = dev(w), dev(e)
    pushes = [(0, 3000, 0, 0), (3000, 6000, 0, 4), (6000, 10000, 4, 12), (10000, 12000, 12, 19)]
    cut = lambda f0, f1: v[:, :, f0:f1].contiguous()  # noqa: E731
    none, one = cut(0, 0), cut(0, 1)

    class TwoSources:
        n_src, training, fused, refinement_module, parameters = 2, False, m.fused, m.refinement_module, m.parameters

    def run(with_refusals):
        pool, out = m.open_streams(2, window=window, hop=hop, max_speakers=2), []
        assert pool.add_face(0) == 0 and pool.add_face(0) == 1
        lone = m.open_streams(1, window=window, hop=hop, max_speakers=1)  # a running stream with its only face
        assert lone.add_face(0) == 0 and tuple(lone.push([0], [x[:10]], [[one[0]]])[0][0].shape) == (0,)
        for a0, a1, f0, f1 in pushes:
            if with_refusals:
                state = lambda: ([pool.counters(s) for s in range(2)], [pool.faces(s) for s in range(2)], [list(b) for b in pool._births])  # noqa: E731
                count, before = lib().load().rtfs_debug_launch_count(), state()
                bad = [([0], [x[:10]], [[one[0]]]), ([0], [x[:10]], [torch.cat([one, one, one])]), ([0], [x[:10]], [one[0]]),  # wrong number of tracks
                       ([0], [x[:10]], [[one[0], cut(0, 2)[1]]]),  # tracks that differ in m
                       ([1], [x[:10]], [[one[0]]]), ([1], [x[:10]], [[]]),  # a slot without faces
                       ([2], [x[:10]], [one]), ([0, 0], [x[:10]] * 2, [one] * 2), ([0], [x[:5121]], [one]), ([0], [x[:10].cpu()], [one]),
                       ([0], [x[:10].double()], [one]), ([0], [x[:10]], [[one[0], one[1].cpu()]])]
                if a0 == 6000:
                    bad.append(([0], [x[:5000]], [none]))  # 6000 + 5000 > 10240 would overwrite what window 0 needs
                for ids, wavs, vids in bad:
                    with pytest.raises(ValueError):
                        pool.push(ids, wavs, vids)
                with pytest.raises(ValueError):
                    pool.add_face(0)  # a full slot
                with pytest.raises(ValueError):
                    lone.drop_face(0, 0)  # the last face of a running stream
                assert lone.faces(0) == [0] and lone.counters(0) == (10, 1, 0, 0)
                with pytest.raises(ValueError):
                    pool.flush([0, 5])
                for kw in (dict(max_speakers=0), dict(max_speakers=17), dict(max_speakers=2, speakers=2), dict(max_speakers=2, sample_rate=48000)):
                    with pytest.raises(ValueError):
                        m.open_streams(2, window=window, hop=hop, **kw)
                from rtfs_net_amd import streaming
                with pytest.raises(ValueError, match="n_src"):
                    streaming.open_face_streams(TwoSources(), 2, 2, window=window, hop=hop)
                assert lib().load().rtfs_debug_launch_count() == count and state() == before
            res = pool.push([0], [x[a0:a1]], [cut(f0, f1)])[0]
            out.append(np.stack([host(res[0]), host(res[1])]))
        res = pool.flush([0])[0]
        out.append(np.stack([host(res[0]), host(res[1])]))
        return np.concatenate(out, axis=1)

    clean = run(False)
    assert np.array_equal(run(True), clean) and clean.shape == (2, 12000)


# ---------------------------------------------------------------- 8. poisoned memory
CASES = "test_framing or test_streams_equal or test_all_planes or test_camera or test_a_slot or test_refusals"
ABNORMAL = (124, 134, 137, 139)


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
def test_poisoned():
    """This file's cases in a fresh child process per pattern, with every workspace / output / state buffer poisoned
    (tests/test_hip_live_speakers.py's discipline: a time limit per child, and no second child after an abnormal exit)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pattern in ("nan", "big"):
        env = dict(os.environ, RTFS_POISON_WS=pattern)
        try:
            pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_live_faces.py"), "-m", "gpu", "-q", "-p",
                                 "no:cacheprovider", "-k", CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s; no further child started")
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            pytest.fail(f"RTFS_POISON_WS={pattern}: abnormal exit status {pr.returncode}; no further child started\n{pr.stdout[-3000:]}")
        assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
