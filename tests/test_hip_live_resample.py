"""Live streams at the microphone's rate on the device (datas.open_resample_streams / ResampleStreamPool, rtfs_live_resample_f32 / _i16,
rtfs_live_resample_reset, the ``sample_rate`` keyword of AVNet.open_streams and System.open_camera_streams / RateStreamPool) against
tests/live_resample_oracle.py:

1. bit-equality: for four rates, concatenated push outputs plus the flush output torch.equal to datas.resample of the whole recording,
   over the edge lengths and one recording of several tiles, three slots on different schedules in one pool, chunk sizes that refill the
   history partly, exactly and wholly, chunks 1-3 elements into their allocation; also against tests/prep_oracle.resample at the two
   bars tests/test_hip_prep.py holds resample to (the worst error is printed; against datas.resample it is exactly 0);
2. int16 PCM chunks at odd 2-byte offsets against the same samples pushed as float32: torch.equal tick by tick;
3. no look-ahead: two recordings that share a prefix give bit-identical outputs for every tick inside the prefix;
4. state: after each tick the current history buffer holds the last 2 width samples received (checked inside every drive); a slot is
   clean after flush and after reset; output blocks start on 128-byte lines;
5. refusals launch nothing and leave no trace;
6. end to end: AVNet.open_streams(sample_rate=48000) against separate_long(datas.resample(wav, 48000), lips) and
   System.open_camera_streams(sample_rate=sr) against System.separate_recording(wav, sr, rois) at the project's bar (rel_err <= 1e-4);
7. drift, the motivating bug: 3 s at 44.1 kHz in chunks of 1000 samples;
8. the cases again in child processes on poisoned memory (RTFS_POISON_WS = nan, big)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import live_resample_oracle as RO
from tests import prep_oracle as PO
from tests.test_hip_longform import dev, host, lib, model
from tests.test_hip_many import video_model
from tests.util import l2_rel, rel_err

pytestmark = pytest.mark.gpu

SPF = 640
POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")
MAX_REL, L2_REL = 1e-4, 1e-5  # the bars of tests/test_hip_prep.py for resample
RATES = [48000, 44100, 8000, 22050]
MC = 7000  # input samples per push: more than one output tile at every rate (a tile is at most 2048 outputs)
LONG = 9001


def D():
    from rtfs_net_amd import datas
    return datas


def offset(x, k):
    """x (float32 or int16) on the device as a view that starts k elements into its allocation."""
    x = np.ascontiguousarray(x)
    return dev(np.concatenate([np.zeros(k, x.dtype), x.reshape(-1)]))[k:]


def drive(pool, P, recs, schedules, check_state=True, raw=None):
    """Stream recs[s] (float32 (L,)) through slot s by per-slot chunk-size lists; ``raw``: slot -> the int16 samples to push in their
    place.  Every tick: shapes, counters, 128-byte lines and, with check_state, the current history buffer.  Returns slot -> the list of
    per-tick outputs (numpy)."""
    counters = {s: (0, 0, 0) for s in range(pool.slots)}
    pos, got, tickno = {s: 0 for s in recs}, {s: [] for s in recs}, 0
    for what, ids, ms in RO.events(schedules):
        flush = what == "flush"
        want = RO.tick(P, counters, ids, ms, pool.max_chunk, flush)
        if flush:
            outs = pool.flush(ids)
        else:
            chunks = []
            for s, m in zip(ids, ms):
                src = recs[s] if raw is None else raw[s]
                chunks.append(offset(src[pos[s]:pos[s] + m], 1 + (tickno + s) % 3 if raw is None else 1 + 2 * ((tickno + s) % 2)))
                pos[s] += m
            outs = pool.push(ids, chunks)
        tickno += 1
        assert len(outs) == len(ids)
        for r, (s, out) in enumerate(zip(ids, outs)):
            lo, hi = want["ranges"][r]
            assert tuple(out.shape) == (hi - lo,) and out.dtype == torch.float32, (what, ids, r)
            if hi > lo:
                assert out.data_ptr() % 128 == 0
            got[s].append(host(out))
            assert pool.counters(s) == want["new"][s][:2] and tuple(pool._counters[s]) == want["new"][s]
        if check_state and not flush:
            hist = host(pool._hist)
            for s in ids:
                a, _, side = want["new"][s]
                for cell, v in RO.history(P, recs[s], a).items():
                    assert hist[s, side, cell].view(np.int32) == np.float32(v).view(np.int32), (what, ids, ms, s, cell)
        counters = want["new"]
    return got


def cycles(P):
    base = RO.sizes(P, MC)
    return [base, base[::-1], [1], [2, 0, P.width], [MC], [2 * P.width - 1, 2 * P.width + 1], [P.o - 1 or 1, P.o + 1]]


def recording(L, seed):
    return (0.3 * np.random.RandomState(seed).randn(L)).astype(np.float32)


_WHOLE = {}


def whole(x, orig):
    """datas.resample of the whole recording, once per recording."""
    key = (orig, x.tobytes())
    if key not in _WHOLE:
        _WHOLE[key] = host(D().resample(dev(x), orig, 16000))
    return _WHOLE[key]


# ---------------------------------------------------------------- 1. bit-equality
@pytest.mark.parametrize("orig", RATES)
def test_streams_are_bit_equal_to_resample_of_the_whole_recording(orig):
    P = RO.Plan(orig, 16000)
    pool = D().open_resample_streams(4, orig, max_chunk=MC)  # slot 3 idle
    Ls, cyc = RO.lengths(P) + [LONG, 2 * MC + 3], cycles(P)
    worst, worst_l2, worst_self = 0.0, 0.0, 0
    for j in range(0, len(Ls), 3):
        L = {s: Ls[(j + s) % len(Ls)] for s in range(3)}
        recs = {s: recording(L[s], 100 * j + s + orig % 97) for s in range(3)}
        # a long recording takes the cycles that hold the maximum (several tiles per push), a short one any
        sch = {s: RO.chunking(L[s], cyc[(j + s) % 2 if L[s] > 1000 else (j + 2 * s) % len(cyc)], start=s) for s in range(3)}
        got = drive(pool, P, recs, sch)
        for s in range(3):
            res, ref, ora = np.concatenate(got[s]), whole(recs[s], orig), PO.resample(recs[s], orig, 16000)
            assert res.shape == ref.shape == ora.shape == (int(lib().load().rtfs_resample_out_len(orig, 16000, L[s])),)
            worst_self = max(worst_self, int(np.abs(res.view(np.int32).astype(np.int64) - ref.view(np.int32)).max()))
            assert torch.equal(torch.from_numpy(res), torch.from_numpy(ref)) and np.array_equal(res.view(np.int32), ref.view(np.int32)), (L[s], s)
            e, l2 = rel_err(res, ora), l2_rel(res, ora)
            worst, worst_l2 = max(worst, e), max(worst_l2, l2)
            assert np.isfinite(res).all() and e <= MAX_REL and l2 <= L2_REL, f"{orig} L {L[s]}: max-rel {e:.3e}, l2-rel {l2:.3e}"
            assert pool.counters(s) == (0, 0)
    print(f"[live resample] {orig}->16000: worst error against datas.resample {worst_self} (bits); against the float64 oracle max-rel "
          f"{worst:.2e}, l2-rel {worst_l2:.2e}")
    assert worst_self == 0


# ---------------------------------------------------------------- 2. int16
@pytest.mark.parametrize("orig", [48000, 44100])
def test_int16_and_float_chunks_agree_bit_for_bit(orig):
    P = RO.Plan(orig, 16000)
    Ls, cyc = [LONG, 2 * P.width + 1, P.o + 1], cycles(P)
    pairs = {s: RO.pcm(np.clip(recording(L, 7 + s), -1.0, 0.999)) for s, L in enumerate(Ls)}
    raw, recs = {s: p[0] for s, p in pairs.items()}, {s: p[1] for s, p in pairs.items()}
    sch = {s: RO.chunking(L, cyc[(2 * s) % len(cyc)], start=s) for s, L in enumerate(Ls)}
    as_float = drive(D().open_resample_streams(3, orig, max_chunk=MC), P, recs, sch)
    as_pcm = drive(D().open_resample_streams(3, orig, max_chunk=MC), P, recs, sch, raw=raw)
    for s in recs:
        assert len(as_float[s]) == len(as_pcm[s])
        for f, i in zip(as_float[s], as_pcm[s]):
            assert torch.equal(torch.from_numpy(f), torch.from_numpy(i))
        assert np.array_equal(np.concatenate(as_pcm[s]), whole(recs[s], orig))


# ---------------------------------------------------------------- 3. no look-ahead
def test_no_look_ahead():
    orig = 44100
    P = RO.Plan(orig, 16000)
    prefix, L = 3000, 4500
    x = recording(L, 31)
    y = np.concatenate([x[:prefix], 5.0 + recording(L - prefix, 32)]).astype(np.float32)
    sizes = RO.chunking(L, [700, 1, 2 * P.width, 999])
    pool = D().open_resample_streams(2, orig, max_chunk=MC)
    got = drive(pool, P, {0: x, 1: y}, {0: sizes, 1: sizes})
    a, inside = 0, 0
    for t, m in enumerate(sizes):
        a += m
        if a <= prefix:
            assert np.array_equal(got[0][t].view(np.int32), got[1][t].view(np.int32)), t
            inside += got[0][t].shape[0]
    assert inside == P.G(max(a for a in np.cumsum(sizes) if a <= prefix)) > 0
    assert not np.array_equal(np.concatenate(got[0]), np.concatenate(got[1]))


# ---------------------------------------------------------------- 4. slot reuse
def stream_once(pool, slot, x, sizes):
    out, a = [], 0
    for m in RO.chunking(x.shape[0], sizes):
        out.append(host(pool.push([slot], [dev(x[a:a + m])])[0]))
        a += m
    out.append(host(pool.flush([slot])[0]))
    return np.concatenate(out)


def test_a_slot_is_clean_after_flush_and_after_reset():
    orig = 48000
    x1, x2, sizes = recording(901, 50), recording(1203, 51), [100, 7, 333]
    fresh = stream_once(D().open_resample_streams(2, orig, max_chunk=MC), 1, x2, sizes)
    pool = D().open_resample_streams(2, orig, max_chunk=MC)
    stream_once(pool, 1, x1, sizes)
    assert np.array_equal(stream_once(pool, 1, x2, sizes), fresh)  # after a flush
    pool.push([1], [dev(x1[:100])])  # a stream dropped half way, on the other side of the history
    assert pool.counters(1) == (100, RO.Plan(orig, 16000).G(100))
    pool.reset([1])
    assert pool.counters(1) == (0, 0)
    assert np.array_equal(stream_once(pool, 1, x2, sizes), fresh)  # after a reset
    assert np.array_equal(fresh, whole(x2, orig)) and np.isfinite(fresh).all()


# ---------------------------------------------------------------- 5. refusals on device tensors
def test_refusals_launch_nothing_and_leave_no_trace():
    orig = 48000
    pool = D().open_resample_streams(2, orig, max_chunk=500)
    x = dev(recording(2000, 70))
    pool.push([0], [x[:300]])
    torch.cuda.synchronize()
    count = lib().load().rtfs_debug_launch_count()
    before = [pool.counters(s) for s in range(2)], pool._hist.clone(), [list(c) for c in pool._counters]
    bad = [([2], [x[:1]]), ([0, 0], [x[:1]] * 2), ([1, 0], [x[:1], x[:501]]), ([0], [x[:1].cpu()]), ([0], [x[:1].double()]),
           ([0, 1], [x[:1], x[:1].to(torch.int16)]), ([0], [x[:4].view(2, 2)]), ([0], [x[0]])]
    for ids, chunks in bad:
        with pytest.raises(ValueError):
            pool.push(ids, chunks)
    with pytest.raises(ValueError):
        pool.flush([0, 5])
    with pytest.raises(ValueError):
        pool.reset([1, 1])
    assert lib().load().rtfs_debug_launch_count() == count
    assert [pool.counters(s) for s in range(2)] == before[0] and [list(c) for c in pool._counters] == before[2]
    assert torch.equal(pool._hist.view(torch.int32), before[1].view(torch.int32))
    rest = torch.cat([pool.push([0], [x[300:800]])[0], pool.flush([0])[0]])  # and the stream goes on as if nothing had been tried
    clean = D().open_resample_streams(1, orig, max_chunk=500)
    first = clean.push([0], [x[:300]])[0]
    assert torch.equal(rest, torch.cat([clean.push([0], [x[300:800]])[0], clean.flush([0])[0]])) and first.shape == (RO.Plan(orig, 16000).G(300),)


# ---------------------------------------------------------------- 6. end to end
def rois(Tv, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(Tv, 96, 96)).astype(np.uint8)


def in_sizes(P, hop, mc):
    f = lambda k: k * P.o // P.n  # noqa: E731
    return [0, 1, f(639), f(640), f(641) + 1, f(hop - 1), f(hop), f(hop) + P.o, f(mc)]


def run_composite(pool, P, wavs, videos, sch, cut):
    """Stream wavs[s] (at the input rate) and videos[s] (frames or embeddings, cut(video, lo, hi) slices them) by the per-slot schedules
    [(m, nf)], flushing each slot in the tick after its last push.  Returns slot -> (n_src, L) at 16 kHz."""
    pos, got = {s: [0, 0] for s in wavs}, {s: [] for s in wavs}
    n = max(len(v) for v in sch.values())
    for i in range(n + 1):
        done = [s for s, v in sch.items() if len(v) == i]
        if done:
            for s, o in zip(done, pool.flush(done)):
                got[s].append(host(o))
        ids = [s for s, v in sch.items() if len(v) > i]
        if ids:
            ms, nf = [sch[s][i][0] for s in ids], [sch[s][i][1] for s in ids]
            outs = pool.push(ids, [offset(wavs[s][pos[s][0]:pos[s][0] + m], 1 + (i + s) % 3) for s, m in zip(ids, ms)],
                             [dev(cut(videos[s], pos[s][1], pos[s][1] + f)) for s, f in zip(ids, nf)])
            for s, m, f, o in zip(ids, ms, nf, outs):
                pos[s][0] += m
                pos[s][1] += f
                got[s].append(host(o))
    return {s: np.concatenate(g, axis=1) for s, g in got.items()}


def input_length(P, L16):
    """The shortest recording at the input rate that resamples to L16 samples."""
    L = (L16 - 1) * P.o // P.n + 1
    assert P.out_len(L) == L16
    return L


@pytest.mark.parametrize("long", [False, True])
def test_audio_streams_at_48k_equal_separate_long_of_the_resampled_recording(long):
    window, hop, mc, orig = 2560, 1280, 2560, 48000
    P = RO.Plan(orig, 16000)
    L16 = 3 * window + 7 if long else window - 1
    L, Tv = input_length(P, L16), -(-L16 // SPF)
    m4 = model(4)
    rng = np.random.RandomState(L16)
    wavs = {s: (0.1 * rng.randn(L)).astype(np.float32) for s in range(3)}
    embs = {s: rng.randn(512, Tv - (2 if s == 1 else 0)).astype(np.float32) for s in range(3)}
    sch = {s: RO.rate_schedule(P, L, embs[s].shape[1], in_sizes(P, hop, mc), mode, window, hop, mc, False, start=s)
           for s, mode in enumerate(("step", "lag", "lead"))}
    pool = m4.open_streams(3, window=window, hop=hop, max_chunk=mc, max_batch=4, sample_rate=orig)
    got = run_composite(pool, P, wavs, embs, sch, lambda v, lo, hi: np.ascontiguousarray(v[:, lo:hi]))
    worst = 0.0
    for s in wavs:
        ref = host(m4.separate_long(D().resample(dev(wavs[s]), orig), dev(embs[s])[None], window=window, hop=hop))[0]
        e = rel_err(got[s], ref)
        worst = max(worst, e)
        assert got[s].shape == ref.shape == (1, L16) and np.isfinite(got[s]).all() and np.abs(ref).max() > 1e-3 and e <= 1e-4, (s, e)
        assert pool.counters(s) == ((0, 0), (0, 0, 0, 0))
    print(f"[live resample] AVNet.open_streams(sample_rate={orig}) L {L16}: worst rel_err vs separate_long(resample(wav)) {worst:.3e}")


@pytest.mark.parametrize("long", [False, True])
@pytest.mark.parametrize("orig,pcm", [(48000, True), (44100, False)])
def test_camera_streams_at_the_microphones_rate_equal_separate_recording(orig, pcm, long):
    import rtfs_net_amd as R
    window, hop, mc = 2560, 1280, 2560
    P = RO.Plan(orig, 16000)
    L16 = 3 * window + 7 if long else window - 1
    L = input_length(P, L16)
    system = R.System(audio_model=model(4), video_model=video_model())
    rng = np.random.RandomState(L16 + orig)
    raw, wavs, tracks, sch = {}, {}, {}, {}
    for s, mode in enumerate(("step", "lag", "lead")):  # slot 1: two frames short
        x = np.clip(0.1 * rng.randn(L), -1.0, 0.999).astype(np.float32)
        raw[s], wavs[s] = RO.pcm(x) if pcm else (x, x)
        tracks[s] = rois(-(-L16 // SPF) - (2 if s == 1 else 0), 80 + s)
        sch[s] = RO.rate_schedule(P, L, tracks[s].shape[0], in_sizes(P, hop, mc), mode, window, hop, mc, True, start=s)
    pool = system.open_camera_streams(3, window=window, hop=hop, max_chunk=mc, max_batch=4, roi_hw=(96, 96), sample_rate=orig)
    got = run_composite(pool, P, raw, tracks, sch, lambda v, lo, hi: v[lo:hi])
    worst = 0.0
    for s in wavs:
        ref = host(system.separate_recording(dev(wavs[s]), orig, dev(tracks[s]), window=window, hop=hop))[0]
        e = rel_err(got[s], ref)
        worst = max(worst, e)
        assert got[s].shape == ref.shape == (1, L16) and np.isfinite(got[s]).all() and np.abs(ref).max() > 1e-3 and e <= 1e-4, (s, e)
        assert pool.counters(s) == ((0, 0), ((0, 0, 0, 0), (0, 0)))
    print(f"[live resample] open_camera_streams(sample_rate={orig}, {'int16' if pcm else 'float32'}) L {L16}: worst rel_err vs "
          f"separate_recording {worst:.3e}")


# ---------------------------------------------------------------- 7. drift
def test_per_chunk_resampling_drifts_and_the_stream_does_not():
    orig, L, m = 44100, 3 * 44100, 1000
    x = recording(L, 90)
    pool = D().open_resample_streams(1, orig, max_chunk=m)
    xd = dev(x)
    outs = [pool.push([0], [xd[a:a + m]])[0] for a in range(0, L, m)] + pool.flush([0])
    res, ref = host(torch.cat(outs)), whole(x, orig)
    expect = int(lib().load().rtfs_resample_out_len(orig, 16000, L))
    per_chunk = sum(int(D().resample(xd[a:a + m], orig).shape[0]) for a in range(0, L, m))
    assert res.shape == (expect,) == ref.shape and expect == 48000 and per_chunk > expect
    assert np.array_equal(res.view(np.int32), ref.view(np.int32))
    print(f"[live resample] 3 s at 44.1 kHz in chunks of {m}: the stream {res.shape[0]} samples, datas.resample per chunk {per_chunk}")


# ---------------------------------------------------------------- 8. poisoned memory
CASES = "test_streams_are or test_int16 or test_no_look or test_a_slot or test_refusals or test_audio_streams or test_camera_streams or test_per_chunk"
ABNORMAL = (124, 134, 137, 139)


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
def test_poisoned():
    """This file's cases in a fresh child process per pattern, with every workspace / output / state buffer poisoned
    (tests/test_hip_live_video.py's discipline: a time limit per child, and no second child after an abnormal exit)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pattern in ("nan", "big"):
        env = dict(os.environ, RTFS_POISON_WS=pattern)
        try:
            pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_live_resample.py"), "-m", "gpu", "-q", "-p",
                                 "no:cacheprovider", "-k", CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s; no further child started")
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            pytest.fail(f"RTFS_POISON_WS={pattern}: abnormal exit status {pr.returncode}; no further child started\n{pr.stdout[-3000:]}")
        assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
