"""Live streams on the fused separator (AVNet.open_streams, StreamPool, rtfs_live_ingest_frame_f32, rtfs_live_overlap_add_f32,
rtfs_live_reset_f32) against tests/live_oracle.py:

1. ingest + framing is a copy: every tick's windows bit-equal to the oracle's, which frames the plain history (no ring), over the small
   plans, three slots with different schedules in the same pushes, chunk tensors that start 4 bytes into an allocation, streams of three
   ring capacities, and the flush form (zeros past L, clamped frames, one slot two frames short);
2. the overlap-add launch against the float64 streaming oracle on synthetic windows, n_src 1 and 2, at test_hip_longform.ola_bound
   (4 ceil(window / hop) 2^-23 max|y| on the y fed to the slot so far: at most ceil(window / hop) float32 multiply-adds and one
   division per sample); hop == window bit-equal;
3. composition with the real forward: == oracle overlap-add of forward on the oracle's batches (ola_bound), and == separate_long of the
   whole recording at the project's bar for forward across batch compositions (tests/util.rel_err <= 1e-4);
4. slot reuse after flush and after reset, bit-equal to a fresh pool;
5. refusals on device tensors launch nothing and leave no trace;
6. the cases again in child processes on poisoned memory (RTFS_POISON_WS = nan, big)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.params import make_inputs
from tests import live_oracle as VO
from tests.test_hip_longform import dev, host, lib, model, ola_bound
from tests.util import rel_err

pytestmark = pytest.mark.gpu

SPF = 640
POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")
PLANS = [(2560, 2560), (2560, 1280), (2560, 640), (1280, 640), (5120, 1920)]
MODES = ("step", "lag", "lead")


class Sized:
    """What open_streams and a StreamPool ask of a model - device, fused path, recurrent cell - taken from the shared R4 model, with an
    n_src of its own to size the buffers.  It has no forward: the synthetic-window tests replace the pool's separator."""
    training = False

    def __init__(self, base, n_src):
        self.n_src, self.fused, self.refinement_module, self.parameters = n_src, base.fused, base.refinement_module, base.parameters


def open_pool(n_src=1, **kw):
    from rtfs_net_amd import streaming
    return streaming.open_streams(Sized(model(4), n_src), **kw)


def offset_view(x):
    """x on the device as a view that starts 4 bytes into its allocation."""
    flat = np.concatenate([np.zeros(1, np.float32), np.ascontiguousarray(x).reshape(-1)])
    return dev(flat)[1:].view(*x.shape)


def drive(pool, xs, vs, events, window, hop, max_chunk, y_of=None, unaligned=True):
    """Stream recordings xs[s] / vs[s] through slot s by ``events``.  With ``y_of`` (row-wise function of the framed windows, numpy) the
    separator is replaced: every tick's framed windows are compared bit for bit against the oracle and y = y_of(windows) goes back, and
    the outputs are compared against the float64 streaming overlap-add at ola_bound.  Returns slot -> concatenated output."""
    n_src = pool.n_src
    counters = {s: (0, 0, 0, 0) for s in xs}
    pos = {s: [0, 0] for s in xs}
    olas = {s: VO.OverlapAdd(window, hop, n_src) for s in xs}
    got = {s: [] for s in xs}
    y_max = {s: 0.0 for s in xs}  # the largest |y| fed to the slot so far: what ola_bound scales with
    seen = {}

    def fake_forward(rows):
        seen["xw"], seen["vw"] = host(pool._xw[:rows]).copy(), host(pool._vw[:rows]).copy()
        seen["y"] = y_of(seen["xw"], seen["vw"]).astype(np.float32)
        pool._y[:rows].copy_(dev(seen["y"]))

    if y_of is not None:
        pool._forward_rows = fake_forward
    put = offset_view if unaligned else dev
    worst = 0.0
    for kind, ids, na, nf in events:
        flush = kind == "flush"
        want = VO.tick(counters, ids, na, nf, window, hop, max_chunk, n_src, flush)
        if flush:
            outs = pool.flush(ids)
        else:
            wavs = [put(xs[s][pos[s][0]:pos[s][0] + n]) for s, n in zip(ids, na)]
            vids = [put(np.ascontiguousarray(vs[s][:, pos[s][1]:pos[s][1] + n])) for s, n in zip(ids, nf)]
            outs = pool.push(ids, wavs, vids)
            for s, n, k in zip(ids, na, nf):
                pos[s][0] += n
                pos[s][1] += k
        assert len(outs) == len(ids)
        if y_of is not None and want["rows"]:
            hist = {s: (xs[s][:pos[s][0]], vs[s][:, :pos[s][1]]) for s in ids}
            exw, evw = VO.frame_rows(want["rows"], hist, {s: tuple(pos[s]) for s in ids}, window, hop)
            assert np.array_equal(seen["xw"], exw), f"audio windows differ in {kind} {ids} {na} {nf} at {counters}"
            assert np.array_equal(seen["vw"], evw), f"video windows differ in {kind} {ids} {na} {nf} at {counters}"
            for i, (s, n) in enumerate(want["rows"]):
                olas[s].feed(n, seen["y"][i])
                y_max[s] = max(y_max[s], float(np.abs(seen["y"][i]).max()))
        for r, (s, out) in enumerate(zip(ids, outs)):
            o, end = want["ranges"][r]
            assert tuple(out.shape) == (n_src, end - o), (kind, ids, r)
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


def synthetic(n_src):
    def y_of(xw, vw):  # row-wise, depends on both inputs
        base = np.tanh(xw) * (1.0 + 0.5 * np.tanh(vw.mean(axis=(1, 2))))[:, None]
        return np.stack([base * (s + 1) for s in range(n_src)], axis=1)
    return y_of


def three_slots(window, hop, max_chunk, seed):
    rng = np.random.RandomState(seed)
    C = VO.capacity(window, max_chunk)
    Ls = [2 * C + hop + 1, window + 3 * hop - 1, window - 1]  # slot 0 wraps its rings twice; slot 2 is one short window
    Tvs = [-(-Ls[0] // SPF), -(-Ls[1] // SPF) - 2, -(-Ls[2] // SPF)]  # slot 1 is two frames short at its flush
    xs = {s: rng.randn(L).astype(np.float32) for s, L in enumerate(Ls)}
    vs = {s: rng.randn(512, Tv).astype(np.float32) for s, Tv in enumerate(Tvs)}
    sizes = VO.chunk_sizes(hop, max_chunk)
    sch = {s: VO.schedule(Ls[s], Tvs[s], sizes, MODES[s], window, hop, max_chunk, start=3 * s + 1) for s in range(3)}
    return xs, vs, VO.events(sch)


# ---------------------------------------------------------------- 1 + 2. the two launches on synthetic windows
@pytest.mark.parametrize("n_src", [1, 2])
@pytest.mark.parametrize("window,hop", PLANS)
def test_ingest_framing_is_a_copy_and_overlap_add_meets_the_oracle(window, hop, n_src):
    pool = open_pool(n_src, slots=3, window=window, hop=hop, max_batch=2)
    xs, vs, events = three_slots(window, hop, window, window + hop + n_src)
    got, worst = drive(pool, xs, vs, events, window, hop, window, y_of=synthetic(n_src))
    for s in xs:
        assert got[s].shape == (n_src, xs[s].shape[0])
    print(f"[live] window {window} hop {hop} n_src {n_src}: {len(events)} ticks, worst overlap-add error {worst:.3f} of the bound")


@pytest.mark.parametrize("n_src", [1, 2])
def test_one_tick_with_three_one_and_no_ready_windows(n_src):
    window, hop = 2560, 640
    pool = open_pool(n_src, slots=3, window=window, hop=hop)
    rng = np.random.RandomState(9 + n_src)
    xs = {s: rng.randn(6000).astype(np.float32) for s in range(3)}
    vs = {s: rng.randn(512, 10).astype(np.float32) for s in range(3)}
    events = [("push", [0, 1, 2], [2559, 2559, 100], [3, 3, 0]), ("push", [2, 0, 1], [100, 1281, 1], [0, 3, 1]),
              ("push", [1, 0, 2], [2560, 640, 2560], [4, 1, 4]), ("flush", [0, 2, 1], None, None)]
    want = VO.tick({0: (2559, 3, 0, 0), 1: (2559, 3, 0, 0), 2: (100, 0, 0, 0)}, [2, 0, 1], [100, 1281, 1], [0, 3, 1], window, hop, window)
    assert want["rows"] == [(0, 0), (0, 1), (0, 2), (1, 0)]
    drive(pool, xs, vs, events, window, hop, window, y_of=synthetic(n_src))


# ---------------------------------------------------------------- 3. composition with the real forward
@pytest.mark.parametrize("hop", [2560, 1920])
def test_streams_equal_separate_long_of_the_whole_recordings(hop):
    m = model(4)
    window, max_chunk, max_batch = 5120, 5120, 2
    Ls = [12000, 5120, 17283]
    xs, vs = {}, {}
    for s, L in enumerate(Ls):
        w, e = make_inputs(1, L, -(-L // SPF), 80 + s)
        xs[s], vs[s] = w[0], e[0]
    sizes = [1, 2561, 639, 0, 5120, 640, 1919, 3000]
    sch = {s: VO.schedule(Ls[s], vs[s].shape[1], sizes, MODES[s], window, hop, max_chunk, start=2 * s) for s in range(3)}
    events = VO.events(sch)
    pool = m.open_streams(3, window=window, hop=hop, max_chunk=max_chunk, max_batch=max_batch)
    got, _ = drive(pool, xs, vs, events, window, hop, max_chunk)
    # forward on exactly the batches the oracle's schedule lists: every tick's rows in chunks of max_batch
    counters, pos = {s: (0, 0, 0, 0) for s in xs}, {s: [0, 0] for s in xs}
    olas, ref = {s: VO.OverlapAdd(window, hop, 1) for s in xs}, {s: [] for s in xs}
    y_max = 0.0
    for kind, ids, na, nf in events:
        want = VO.tick(counters, ids, na, nf, window, hop, max_chunk, 1, kind == "flush")
        if kind == "push":
            for s, n, k in zip(ids, na, nf):
                pos[s][0] += n
                pos[s][1] += k
        if want["rows"]:
            hist = {s: (xs[s][:pos[s][0]], vs[s][:, :pos[s][1]]) for s in ids}
            xw, vw = VO.frame_rows(want["rows"], hist, {s: tuple(pos[s]) for s in ids}, window, hop)
            with torch.no_grad():
                y = np.concatenate([host(m(dev(xw[c:c + max_batch]), dev(vw[c:c + max_batch]))) for c in range(0, len(want["rows"]), max_batch)])
            y_max = max(y_max, float(np.abs(y).max()))
            for i, (s, n) in enumerate(want["rows"]):
                olas[s].feed(n, y[i])
        for s, (o, end) in zip(ids, want["ranges"]):
            ref[s].append(olas[s].take(o, end))
        counters = want["new"]
    for s, L in enumerate(Ls):
        want = np.concatenate(ref[s], axis=1)
        err, bound = float(np.abs(got[s] - want).max()), ola_bound(window, hop, np.float64(y_max))
        whole = host(m.separate_long(dev(xs[s][None]), dev(vs[s][None]), window=window, hop=hop))[0]
        e = rel_err(got[s], whole)
        print(f"[live] hop {hop} slot {s} L {L}: vs oracle overlap-add of forward on the tick batches {err:.3e} (bound {bound:.3e}); "
              f"vs separate_long(whole) max-rel {e:.3e}")
        assert got[s].shape == (1, L) and np.isfinite(got[s]).all() and err <= bound, (s, err, bound)
        assert e <= 1e-4, (s, e)


# ---------------------------------------------------------------- 4. slot reuse
def stream_once(pool, slot, x, v, sizes, window, hop):
    out, a, f = [], 0, 0
    for na, nf in VO.schedule(x.shape[0], v.shape[1], sizes, "step", window, hop, window):
        out.append(host(pool.push([slot], [dev(x[a:a + na])], [dev(np.ascontiguousarray(v[:, f:f + nf]))])[0]))
        a, f = a + na, f + nf
    out.append(host(pool.flush([slot])[0]))
    return np.concatenate(out, axis=1)


def test_a_slot_is_clean_after_flush_and_after_reset():
    m, window, hop = model(4), 5120, 2560
    (w1, e1), (w2, e2) = make_inputs(1, 9000, 15, 91), make_inputs(1, 13001, 21, 92)
    sizes = [2000, 640, 3333]
    fresh = stream_once(m.open_streams(2, window=window, hop=hop), 1, w2[0], e2[0], sizes, window, hop)
    pool = m.open_streams(2, window=window, hop=hop)
    stream_once(pool, 1, w1[0], e1[0], sizes, window, hop)
    assert np.array_equal(stream_once(pool, 1, w2[0], e2[0], sizes, window, hop), fresh)  # after a flush
    pool.push([1], [dev(w1[0, :4000])], [dev(np.ascontiguousarray(e1[0, :, :6]))])  # a stream dropped half way, sums pending
    pool.push([1], [dev(w1[0, 4000:7000])], [dev(np.ascontiguousarray(e1[0, :, 6:11]))])
    assert pool.counters(1)[2] == 1
    pool.reset([1])
    assert pool.counters(1) == (0, 0, 0, 0)
    assert np.array_equal(stream_once(pool, 1, w2[0], e2[0], sizes, window, hop), fresh)  # after a reset
    assert fresh.shape == (1, 13001) and np.isfinite(fresh).all()


# ---------------------------------------------------------------- 5. refusals on device tensors
def test_refusals_launch_nothing_and_leave_no_trace():
    m, window, hop = model(4), 5120, 2560
    w, e = make_inputs(1, 12000, 19, 93)
    x, v = dev(w[0]), dev(e[0])
    pushes = [(0, 3000, 0, 0), (3000, 6000, 0, 4), (6000, 10000, 4, 12), (10000, 12000, 12, 19)]  # the video lags, then catches up
    none, one = v[:, :0].contiguous(), v[:, :1].contiguous()

    def run(with_refusals):
        pool, out = m.open_streams(2, window=window, hop=hop), []
        for a0, a1, f0, f1 in pushes:
            if with_refusals:
                count, before = lib().load().rtfs_debug_launch_count(), [pool.counters(s) for s in range(2)]
                bad = [([2], [x[:10]], [none]), ([0, 0], [x[:10]] * 2, [one] * 2), ([1, 0], [x[:10], x[:5121]], [one, one]),
                       ([0], [x[:10].cpu()], [one]), ([0], [x[:10].double()], [one]), ([0], [x[:10]], [v[:500, :1].contiguous()])]
                if a0 == 6000:  # 6000 samples, 4 frames, no window yet: 6000 + 5000 > 10240 would overwrite what window 0 needs
                    bad.append(([1, 0], [x[:10], x[:5000]], [one, none]))
                for ids, wavs, vids in bad:
                    with pytest.raises(ValueError):
                        pool.push(ids, wavs, vids)
                with pytest.raises(ValueError):
                    pool.flush([0, 5])
                assert lib().load().rtfs_debug_launch_count() == count and [pool.counters(s) for s in range(2)] == before
            out.append(host(pool.push([0], [x[a0:a1]], [v[:, f0:f1].contiguous()])[0]))
        out.append(host(pool.flush([0])[0]))
        return np.concatenate(out, axis=1)

    clean = run(False)
    assert np.array_equal(run(True), clean) and clean.shape == (1, 12000)


# ---------------------------------------------------------------- 6. poisoned memory
CASES = "test_ingest or test_one_tick or test_streams_equal or test_a_slot or test_refusals"
ABNORMAL = (124, 134, 137, 139)


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
def test_poisoned():
    """This file's cases in a fresh child process per pattern, with every workspace / output / state buffer poisoned
    (tests/test_hip_longform.py's discipline: a time limit per child, and no second child after an abnormal exit)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for pattern in ("nan", "big"):
        env = dict(os.environ, RTFS_POISON_WS=pattern)
        try:
            pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_live.py"), "-m", "gpu", "-q", "-p",
                                 "no:cacheprovider", "-k", CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s; no further child started")
        if pr.returncode < 0 or pr.returncode in ABNORMAL:
            pytest.fail(f"RTFS_POISON_WS={pattern}: abnormal exit status {pr.returncode}; no further child started\n{pr.stdout[-3000:]}")
        assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
