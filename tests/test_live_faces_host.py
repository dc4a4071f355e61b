"""Host side of live streaming with faces that come and go (AVNet.open_streams(max_speakers=Kmax), FaceStreamPool,
rtfs_live_faces_plan) against tests/live_faces_oracle.py: the tick arithmetic of the C planner over seeded random schedules with joins
and drops, every refusal with its reason and with the outputs unwritten, the fixed-K planner as the special case of all births 0, the
class end to end on CPU tensors with a cheap row-wise separator against a single-track CPU ``StreamPool`` started at each face's birth,
and every refusal of add_face / drop_face / push with all state unchanged.  None of it touches a device.

``Runner`` drives a pool and the oracle side by side through a list of events; tests/test_hip_live_faces.py uses it on the device."""
import ctypes

import numpy as np
import pytest
import torch

from tests import live_faces_oracle as FO
from tests import live_oracle as VO
from tests.test_live_host import _model, c_tick, lib, three_slot_events
from tests.test_live_speakers_host import _cheap

SPF = 640
PLANS = [(2560, 2560), (2560, 1280), (2560, 640), (1280, 640), (5120, 1920)]  # the PLANS of tests/test_hip_live.py
LL = ctypes.c_longlong
SENTINEL = -7


def c_plan(counters, births, ids, na, nf, slots, window, hop, max_chunk, Kmax, flush, row_cap=64):
    """rtfs_live_faces_plan on the named slots -> (rc, new counters of the named slots, table, row_counts, sizes, refused); every output
    is prefilled with SENTINEL."""
    R, Kw = len(ids), max(1, min(Kmax, 16))
    words = 15 + 2 * Kw
    cnt = [v for s in ids for v in counters.get(s, (0, 0, 0, 0))]
    bs = [b for s in ids for b in births.get(s, [-1] * Kw)[:Kw]]
    new, table, rcs = (LL * (4 * R))(*([SENTINEL] * 4 * R)), (LL * (words * R))(*([SENTINEL] * words * R)), (LL * max(row_cap, 1))(*([SENTINEL] * max(row_cap, 1)))
    sizes, refused = (LL * 6)(*([SENTINEL] * 6)), (ctypes.c_int * 2)(SENTINEL, SENTINEL)
    rc = lib().rtfs_live_faces_plan((LL * R)(*ids), (LL * (4 * R))(*cnt), None if flush else (LL * R)(*na), None if flush else (LL * R)(*nf), R,
                                    slots, int(flush), window, hop, max_chunk, Kmax, (LL * len(bs))(*bs), row_cap, new, table, rcs, sizes, refused)
    return rc, [tuple(new[4 * r:4 * r + 4]) for r in range(R)], list(table), list(rcs), list(sizes), tuple(refused)


def compare(counters, births, ids, na, nf, slots, window, hop, max_chunk, Kmax, flush, row_cap=64):
    """The C planner against the oracle on one call; -> the oracle's tick, or None for a refusal (same index, same reason, every
    output still unwritten)."""
    got = c_plan(counters, births, ids, na, nf, slots, window, hop, max_chunk, Kmax, flush, row_cap)
    try:
        want = FO.tick(counters, births, ids, na, nf, window, hop, max_chunk, Kmax, flush, row_cap)
    except FO.Refused as why:
        assert got[0] == -4 and got[5] == (why.r, why.reason), (got[0], got[5], str(why), ids, na, nf, flush)
        assert all(v == SENTINEL for out in got[1] for v in out) and all(v == SENTINEL for out in got[2:5] for v in out), "a refusal wrote"
        return None
    assert got[0] == 0 and got[5] == (-1, 0), (got[0], got[5], ids, na, nf, flush)
    assert got[1] == [want["new"][s] for s in ids]
    assert got[2] == want["table"], (got[2], want["table"])
    assert got[3][:len(want["row_counts"])] == want["row_counts"] and got[4] == want["sizes"]
    return want


def apply_face_event(ev, counters, births, hop):
    kind, s, j = ev
    if kind == "add":
        j = min(k for k, b in enumerate(births[s]) if b < 0) if j is None else j
        assert births[s][j] < 0
        births[s][j] = FO.birth_at(counters[s][1], hop)
    else:
        assert births[s][j] >= 0
        births[s][j] = -1
    return j


@pytest.mark.parametrize("window,hop", PLANS)
def test_planner_against_the_oracle_over_random_schedules(window, hop):
    slots, Kmax, max_chunk = 3, 3, window
    refusals, mixed = set(), 0
    for seed in range(4):
        rng = np.random.RandomState(1000 * seed + window + hop)
        events = FO.merge(FO.random_scripts(rng, slots, Kmax, window, hop, max_chunk, pushes=14))
        counters, births = {s: (0, 0, 0, 0) for s in range(slots)}, {s: [-1] * Kmax for s in range(slots)}
        args = (slots, window, hop, max_chunk, Kmax)
        for ev in events:
            if ev[0] in ("add", "drop"):
                apply_face_event(ev, counters, births, hop)
                continue
            kind, ids, na, nf = ev
            if kind == "push":  # calls that must be refused, from this very state
                one = [0] * len(ids)
                bad = [([slots], [0], [0]), ([-1], [0], [0]), (ids + ids[:1], na + na[:1], nf + nf[:1]), (ids, [max_chunk + 1] + na[1:], nf),
                       (ids, na, nf[:-1] + [max_chunk // SPF + 1]), (ids, [-1] + na[1:], nf), (ids, [max_chunk] * len(ids), one),
                       (ids, one, [max_chunk // SPF] * len(ids))]
                for b_ids, b_na, b_nf in bad:  # the last two are refused once a side is a chunk too far ahead
                    compare(counters, births, b_ids, b_na, b_nf, *args, False)
                empty = [s for s in range(slots) if s not in ids and not any(b >= 0 for b in births[s])]
                if empty:
                    assert compare(counters, births, ids + empty[:1], na + [0], nf + [0], *args, False) is None
                    refusals.add(FO.NO_FACES)
                late = dict(births)
                late[ids[0]] = [FO.birth_at(counters[ids[0]][1], hop) + 1] + births[ids[0]][1:]
                assert compare(counters, late, ids, na, nf, *args, False) is None  # a birth no add_face can have set
                for Kbad in (0, 17):
                    assert compare(counters, births, ids, na, nf, slots, window, hop, max_chunk, Kbad, False) is None
            if kind == "flush" and compare(counters, births, ids, na, nf, *args, True) is None:
                ok = []  # a slot with samples in which no face takes part: refused whole; slot by slot the others pass, it is reset
                for s in ids:
                    if compare(counters, births, [s], None, None, *args, True) is None:
                        counters[s], births[s] = (0, 0, 0, 0), [-1] * Kmax
                        refusals.add(FO.NO_FRAMES)
                    else:
                        ok.append(s)
                ids = ok
                if not ids:
                    continue
            want = compare(counters, births, ids, na, nf, *args, kind == "flush")
            assert want is not None
            if want["rows"]:
                assert compare(counters, births, ids, na, nf, *args, kind == "flush", row_cap=len(want["rows"]) - 1) is None  # too few rows
            mixed += len(set(want["row_counts"])) > 1
            counters = want["new"]
            if kind == "flush":
                for s in ids:
                    births[s] = [-1] * Kmax
    assert mixed > 0, "no tick with windows of different target counts"
    print(f"[live faces host] window {window} hop {hop}: {mixed} ticks with ragged row_counts; extra refusal reasons met {sorted(refusals)}")


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("window,hop", PLANS)
def test_all_births_zero_is_the_fixed_k_planner(window, hop, K):
    max_chunk = window
    counters, births = {s: (0, 0, 0, 0) for s in range(3)}, {s: [0] * K for s in range(3)}
    for kind, ids, na, nf in three_slot_events(window, hop, max_chunk):
        flush = kind == "flush"
        rc, new, table, sizes, refused = c_tick(counters, ids, na, nf, 3, window, hop, max_chunk, K, flush)
        got = c_plan(counters, births, ids, na, nf, 3, window, hop, max_chunk, K, flush)
        assert rc == 0 and got[0] == 0
        R = len(ids)
        assert got[2][:13 * R] == table and got[1] == new
        assert got[2][13 * R:14 * R] == [0 if (flush and counters[s][0] == 0) else K for s in ids]
        assert got[2][14 * R:15 * R] == [K * r0 for r0 in table[7 * R:8 * R]]
        assert [got[4][i] for i in (0, 2, 3, 4, 5)] == sizes and got[4][1] == K * sizes[0] and got[3][:sizes[0]] == [K] * sizes[0]
        for s, c in zip(ids, new):
            counters[s] = c


# ---------------------------------------------------------------- a pool and the oracle side by side
class Runner:
    """Drives a FaceStreamPool and the oracle through events [("add", slot, plane | None) | ("drop", slot, plane) | ("push", ids, na, nf)
    | ("flush", ids, None, None)] with seeded random data.  ``put`` brings a numpy array to the pool's device, ``host`` a tensor back.
    With ``y_of`` (row-wise function of the audio window, the target's own lips and its face id, numpy) the separator is replaced:
    every tick's framed windows are compared bit for bit with the oracle's, the outputs with the float64 streaming overlap-add of each
    face at ``bound(window, hop, max |y| fed to the face)``, bit for bit at hop == window.  Every face that ends (dropped or flushed)
    is kept in ``closed`` with its outputs, its birth and the slot's stream.  With ``sep`` (the real separator on the oracle's own framed
    windows: (xw, vw, row_counts) -> y) the same overlap-add comparison runs without replacing anything.  ``draw`` = (audio(slot, a0, n),
    lips(slot, plane, f0, m)) supplies the data instead of the seeded generator."""

    def __init__(self, pool, slots, Kmax, window, hop, max_chunk, seed, put, host, stacked=False, y_of=None, bound=None, sep=None, draw=None):
        self.pool, self.Kmax, self.window, self.hop, self.max_chunk = pool, Kmax, window, hop, max_chunk
        self.put, self.host, self.stacked, self.y_of, self.bound, self.sep, self.draw = put, host, stacked, y_of, bound, sep, draw
        self.rng = np.random.RandomState(seed)
        self.counters = {s: (0, 0, 0, 0) for s in range(slots)}
        self.births = {s: [-1] * Kmax for s in range(slots)}
        self.hx = {s: np.zeros(0, np.float32) for s in range(slots)}
        self.hv, self.live, self.log = {s: {} for s in range(slots)}, {s: {} for s in range(slots)}, {s: [] for s in range(slots)}
        self.closed, self.worst, self.ticks = [], 0.0, 0
        self.seen = dict(ragged=0, empty_audio=0, empty_video=0, reused_plane_stale=0, join_off_hop_pending=0, both_sides=0, no_frame_face=0,
                         wraps={s: 0 for s in range(slots)}, three_from_start=set())
        self.last_planes = {s: set() for s in range(slots)}  # planes a face of the CURRENT stream has held, with sums or frames in them
        if y_of is not None:
            pool._forward_targets = self._fake

    # the separator replaced: compare the framed windows, hand back y_of
    def _fake(self, row_counts):
        want, pool = self.want, self.pool
        assert list(row_counts) == want["row_counts"]
        rows, T = len(row_counts), sum(row_counts)
        xw, vw = self.host(pool._xw[:rows]).copy(), self.host(pool._vw[:T]).copy()
        exw, evw = FO.frame_rows(want["rows"], want["targets"], self.hist, self.limits, self.window, self.hop)
        assert np.array_equal(xw, exw), f"audio windows differ at {self.counters}"
        assert np.array_equal(vw, evw), f"video windows differ at {self.counters} births {self.births}"
        js = np.array([j for _, _, j in want["targets"]], np.int64)
        self.y = self.y_of(xw[np.repeat(np.arange(rows), row_counts)], vw, js).astype(np.float32) if T else np.zeros((0, self.window), np.float32)
        if T:
            pool._yt[:T].copy_(self.put(self.y))
        self.faked = True

    def _close(self, s, j, state):
        rec = self.live[s].pop(j)
        rec.update(state=state, x=self.hx[s].copy(), v=self.hv[s].pop(j), pushes=self.log[s][rec["log0"]:], c_end=self.counters[s])
        self.closed.append(rec)

    def run(self, events):
        for ev in events:
            self.step(ev)
        return self

    def step(self, ev):
        pool, W, H = self.pool, self.window, self.hop
        Hv = H // SPF
        if ev[0] == "add":
            _, s, j = ev
            a, f, e, o = self.counters[s]
            got = pool.add_face(s) if j is None else pool.add_face(s, j)
            j = apply_face_event(ev, self.counters, self.births, H)
            assert got == j and pool.faces(s) == [k for k, b in enumerate(self.births[s]) if b >= 0]
            b = self.births[s][j]
            assert pool.birth(s, j) == b >= e
            if j in self.last_planes[s] and e > 0:
                self.seen["reused_plane_stale"] += 1  # the plane holds the previous occupant's frames and pending sums
            if f % Hv and e < b:
                self.seen["join_off_hop_pending"] += 1
            if f == 0 and a == 0 and sum(k >= 0 for k in self.births[s]) == 3:
                self.seen["three_from_start"].add(s)
            self.hv[s][j] = np.full((512, f), np.nan, np.float32)
            self.live[s][j] = dict(s=s, j=j, b=b, a_add=a, f_add=f, log0=len(self.log[s]), got=[], ola=FO.OverlapAdd(W, H, b), y_max=0.0)
            self.last_planes[s].add(j)
            return
        if ev[0] == "drop":
            _, s, j = ev
            pool.drop_face(s, j)
            apply_face_event(ev, self.counters, self.births, H)
            self._close(s, j, "dropped")
            assert pool.faces(s) == [k for k, b in enumerate(self.births[s]) if b >= 0]
            return
        kind, ids, na, nf = ev
        flush = kind == "flush"
        if flush:
            try:
                FO.tick(self.counters, self.births, ids, na, nf, W, H, self.max_chunk, self.Kmax, True)
            except FO.Refused as why:  # a slot with samples in which no face takes part: refused whole, then slot by slot
                assert why.reason == FO.NO_FRAMES
                before = [(pool.counters(s), pool.faces(s)) for s in ids]
                with pytest.raises(ValueError, match="no video frame"):
                    pool.flush(ids)
                assert [(pool.counters(s), pool.faces(s)) for s in ids] == before
                for s in ids:
                    try:
                        FO.tick(self.counters, self.births, [s], None, None, W, H, self.max_chunk, self.Kmax, True)
                    except FO.Refused:
                        with pytest.raises(ValueError):
                            pool.flush([s])
                        pool.reset([s])
                        for j in list(self.live[s]):
                            self._close(s, j, "reset")
                        self._end_stream(s)
                    else:
                        self.step(("flush", [s], None, None))
                return
        want = self.want = FO.tick(self.counters, self.births, ids, na, nf, W, H, self.max_chunk, self.Kmax, flush)
        self.ticks += 1
        self.seen["ragged"] += any(len({c for (s2, _), c in zip(want["rows"], want["row_counts"]) if s2 == s}) > 1 for s in ids)
        for s, present in zip(ids, want["present"]):
            ns = [n for s2, n in want["rows"] if s2 == s]
            if ns and any(ns[0] < b <= ns[-1] for _, b in present):
                self.seen["both_sides"] += 1
        if not flush:
            wavs, vids = [], []
            for s, n, m in zip(ids, na, nf):
                x = self.draw[0](s, self.counters[s][0], n) if self.draw else self.rng.randn(n).astype(np.float32)
                self.hx[s] = np.concatenate([self.hx[s], x])
                wavs.append(self.put(x))
                cut = np.stack([self.draw[1](s, j, self.counters[s][1], m) if self.draw else self.rng.randn(512, m).astype(np.float32)
                                for j in sorted(self.live[s])])
                for i, j in enumerate(sorted(self.live[s])):
                    self.hv[s][j] = np.concatenate([self.hv[s][j], cut[i]], axis=1)
                vids.append(self.put(cut) if self.stacked else [self.put(cut[i]) for i in range(cut.shape[0])])
                self.log[s].append((self.counters[s][0] + n, self.counters[s][1] + m))
                self.seen["empty_audio"] += n == 0
                self.seen["empty_video"] += m == 0
        self.limits = {s: (self.hx[s].shape[0], self.counters[s][1] + (0 if flush else nf[ids.index(s)])) for s in ids}
        self.hist = {s: (self.hx[s], self.hv[s]) for s in ids}
        self.faked = False
        outs = pool.flush(ids) if flush else pool.push(ids, wavs, vids)
        assert len(outs) == len(ids)
        if self.y_of is not None:
            assert self.faked == bool(want["rows"])
        elif self.sep is not None and want["targets"]:
            self.y = self.sep(*FO.frame_rows(want["rows"], want["targets"], self.hist, self.limits, W, H), want["row_counts"])
        if self.y_of is not None or self.sep is not None:
            for t, (s, n, j) in enumerate(want["targets"]):
                rec = self.live[s][j]
                rec["ola"].feed(n, self.y[t])
                rec["y_max"] = max(rec["y_max"], float(np.abs(self.y[t]).max()))
        C = VO.capacity(W, self.max_chunk)
        for r, (s, out) in enumerate(zip(ids, outs)):
            assert sorted(out) == sorted(self.live[s]), (kind, s, sorted(out), sorted(self.live[s]))
            o, end = want["ranges"][r]
            for i, j in enumerate(sorted(out)):
                rec, (lo, hi) = self.live[s][j], want["face_ranges"][r].get(j, (0, 0))
                assert tuple(out[j].shape) == (hi - lo,) and out[j].dtype == torch.float32, (kind, s, j, tuple(out[j].shape), lo, hi)
                res = self.host(out[j])
                rec["got"].append(res)
                if j not in want["face_ranges"][r]:
                    self.seen["no_frame_face"] += flush and rec["f_add"] == self.counters[s][1]
                    continue
                if out[j].is_cuda and hi > lo and lo == o and want["present"][r][0][0] == j:
                    assert out[j].data_ptr() % 128 == 0, (kind, s, j)  # every slot's block starts on a 128-byte line
                if (self.y_of is not None or self.sep is not None) and hi > lo:
                    ref = rec["ola"].take(lo, hi)
                    err, bound = float(np.abs(res - ref).max()), self.bound(W, H, np.float64(rec["y_max"]))
                    assert np.isfinite(res).all() and err <= bound, (kind, s, j, err, bound)
                    self.worst = max(self.worst, err / bound)
                    if H == W and self.y_of is not None:
                        assert np.array_equal(res, ref.astype(np.float32)), (kind, s, j)
            assert pool.counters(s) == want["new"][s]
        for s in ids:
            self.seen["wraps"][s] = max(self.seen["wraps"][s], self.limits[s][0] // C)
        self.counters = want["new"]
        if flush:
            for s in ids:
                for j in list(self.live[s]):
                    self._close_flushed(s, j, want, ids.index(s))
                self._end_stream(s)
                assert pool.faces(s) == []

    def _close_flushed(self, s, j, want, r):
        took_part = j in want["face_ranges"][r]
        rec = self.live[s].pop(j)
        rec.update(state="flushed" if took_part else "idle", x=self.hx[s].copy(), v=self.hv[s].pop(j), pushes=self.log[s][rec["log0"]:],
                   c_end=(self.limits[s][0], self.limits[s][1], 0, 0))
        self.closed.append(rec)

    def _end_stream(self, s):
        self.counters = {**self.counters, s: (0, 0, 0, 0)}
        self.births[s] = [-1] * self.Kmax
        self.hx[s], self.hv[s], self.log[s], self.last_planes[s] = np.zeros(0, np.float32), {}, [], set()


def replay_single(single, rec, window, hop, max_chunk, put, host):
    """What a single-track StreamPool started at the face's birth gives: the slot's audio from sample b hop and the face's lips from
    frame b hop / 640, cut as the slot's pushes cut them (what had arrived before the add first, in pieces of max_chunk), flushed if the
    face was; -> the concatenated output (L',)."""
    b, x, v = rec["b"], rec["x"], rec["v"]
    pa, pf, out = b * hop, b * hop // SPF, []
    none = np.zeros((512, 0), np.float32)
    while pa < rec["a_add"]:
        n = min(max_chunk, rec["a_add"] - pa)
        out.append(host(single.push([0], [put(x[pa:pa + n])], [put(none)])[0]))
        pa += n
    for a, f in rec["pushes"]:
        a, f = max(a, pa), max(f, pf)
        out.append(host(single.push([0], [put(x[pa:a])], [put(np.ascontiguousarray(v[:, pf:f]))])[0]))
        pa, pf = a, f
    if rec["state"] == "flushed":
        out.append(host(single.flush([0])[0]))
    else:
        single.reset([0])
    return np.concatenate(out, axis=1)[0] if out else np.zeros(0, np.float32)


@pytest.mark.parametrize("window,hop", [(2560, 2560), (2560, 640), (5120, 1920)])
def test_pool_on_cpu_tensors_equals_a_single_track_pool_started_at_the_birth(window, hop):
    """Every window the pool frames is a copy and the separator is row-wise, so a face's output differs from the single-track pool's by
    the float32 cross-fade only: 4 ceil(window / hop) 2^-23 max|y|, the bound tests/test_live_speakers_host.py uses; hop == window is
    bit-equal."""
    m = _model()
    seen = [0.0]

    def forward_modular(wav, emb):
        y = _cheap(wav, emb)
        seen[0] = max(seen[0], float(y.abs().max()))
        return y

    m.forward_modular = forward_modular
    slots, Kmax, max_chunk = 3, 3, window
    pool = m.open_streams(slots, window=window, hop=hop, max_chunk=max_chunk, max_batch=4, max_speakers=Kmax)
    import rtfs_net_amd as R
    assert type(pool) is R.FaceStreamPool and type(R.System(audio_model=m).open_streams(slots=1, window=1280, hop=640, max_speakers=2)) is R.FaceStreamPool
    assert pool._aring.numel() * 4 + pool._vring.numel() * 4 + pool._acc.numel() * 4 == slots * (4 * pool.capacity * (1 + Kmax) + 2048 * Kmax * pool.capacity // 640)
    single = m.open_streams(1, window=window, hop=hop, max_chunk=max_chunk, max_batch=4)
    host = lambda t: t.numpy()  # noqa: E731
    checked = dict(dropped=0, flushed=0, idle=0, reset=0)
    for seed in range(3):
        rng = np.random.RandomState(77 * seed + window + hop)
        run = Runner(pool, slots, Kmax, window, hop, max_chunk, seed, torch.from_numpy, host, stacked=bool(seed % 2))
        run.run(FO.merge(FO.random_scripts(rng, slots, Kmax, window, hop, max_chunk, pushes=12)))
        bound = 4 * -(-window // hop) * 2.0 ** -23 * seen[0]
        for rec in run.closed:
            got = np.concatenate(rec["got"]) if rec["got"] else np.zeros(0, np.float32)
            checked[rec["state"]] += 1
            if rec["state"] in ("idle", "reset") and got.shape[0] == 0:
                continue
            want = replay_single(single, rec, window, hop, max_chunk, torch.from_numpy, host)
            assert got.shape == want.shape, (rec["s"], rec["j"], rec["b"], rec["state"], got.shape, want.shape)
            if got.shape[0]:
                err = float(np.abs(got - want).max())
                assert err <= bound, (rec["s"], rec["j"], rec["b"], err, bound)
                if hop == window:
                    assert np.array_equal(got, want)
    assert checked["dropped"] and checked["flushed"], checked
    print(f"[live faces host] window {window} hop {hop}: faces checked {checked}")


def test_refusals_leave_all_state_unchanged():
    m = _model()
    m.forward_modular = _cheap
    for kw in (dict(max_speakers=0), dict(max_speakers=17), dict(max_speakers=2.0), dict(max_speakers=True), dict(max_speakers=2, speakers=2),
               dict(max_speakers=2, sample_rate=48000), dict(max_speakers=2, window=2561), dict(max_speakers=2, max_chunk=641),
               dict(max_speakers=16, max_chunk=(1 << 20) // 640 * 640)):
        with pytest.raises(ValueError):
            m.open_streams(**dict(dict(slots=2, window=2560, hop=1280), **kw))
    m2 = _model()
    m2.n_src = 2
    with pytest.raises(ValueError, match="n_src"):
        m2.open_streams(2, window=2560, hop=1280, max_speakers=2)
    pool = m.open_streams(3, window=2560, hop=1280, max_batch=2, max_speakers=2)
    a, t3, t2 = torch.zeros(2000), torch.zeros(512, 3), torch.zeros(512, 2)
    assert pool.add_face(0) == 0 and pool.add_face(0) == 1 and pool.add_face(2, 1) == 1
    out = pool.push([0, 2], [a, a], [torch.zeros(2, 512, 3), [t3]])
    assert [{j: tuple(v.shape) for j, v in d.items()} for d in out] == [{0: (0,), 1: (0,)}, {1: (0,)}]
    state = lambda: ([pool.counters(s) for s in range(3)], [pool.faces(s) for s in range(3)], [list(b) for b in pool._births])  # noqa: E731
    before = state()
    assert before[:2] == ([(2000, 3, 0, 0), (0, 0, 0, 0), (2000, 3, 0, 0)], [[0, 1], [], [1]])
    for call in (lambda: pool.add_face(0), lambda: pool.add_face(0, 1), lambda: pool.add_face(2, 2), lambda: pool.add_face(3), lambda: pool.add_face(2, -1),
                 lambda: pool.add_face(1.5), lambda: pool.drop_face(2, 1), lambda: pool.drop_face(2, 0), lambda: pool.drop_face(1, 0),
                 lambda: pool.drop_face(0, 2), lambda: pool.faces(5)):
        with pytest.raises(ValueError):
            call()
        assert state() == before
    bad = [([1], [a], [[t3]]), ([1], [a], [[]]),  # a slot without faces
           ([0], [a], [[t3]]), ([0], [a], [[t3, t3, t3]]), ([0], [a], [torch.zeros(1, 512, 3)]), ([0], [a], [t3]), ([2], [a], [[t3, t3]]),  # wrong count
           ([0], [a], [[t3, t2]]),  # tracks that differ in m
           ([3], [a], [[t3]]), ([0, 0], [a, a], [[t3, t3], [t3, t3]]), ([0, 2], [a], [[t3, t3], [t3]]), ([2, 0], [a, torch.zeros(2561)], [[t3], [t3, t3]]),
           ([0], [a.double()], [[t3, t3]]), ([0], [a], [[t3, t3.double()]]), ([0], [a], [[t3, None]])]
    for ids, wavs, vids in bad:
        with pytest.raises(ValueError):
            pool.push(ids, wavs, vids)
        assert state() == before, (ids,)
    with pytest.raises(ValueError):
        pool.flush([0, 0])
    pool.add_face(1)
    with pytest.raises(ValueError, match="no video frame"):  # samples, and a face without a frame
        pool.push([1], [a], [[torch.zeros(512, 0)]]) and pool.flush([1, 0])
    assert pool.counters(0) == (2000, 3, 0, 0) and pool.counters(1) == (2000, 0, 0, 0) and pool.faces(1) == [0]
    pool.reset([1])
    assert pool.faces(1) == [] and pool.counters(1) == (0, 0, 0, 0)
    pool.drop_face(0, 0)  # not the last
    assert pool.faces(0) == [1]
    res = pool.flush([0, 1, 2])
    assert [{j: tuple(v.shape) for j, v in d.items()} for d in res] == [{1: (2000,)}, {}, {1: (2000,)}]
    assert [pool.faces(s) for s in range(3)] == [[], [], []]


def test_launchers_refuse_bad_sizes_and_skip_an_empty_tick_without_a_device():
    """Both launchers check their arguments before anything touches a device: Kmax outside 1 .. 16, sizes the planner refuses and
    misaligned buffers are -4, and a tick in which nothing arrived and nothing is ready is RTFS_OK without a launch."""
    L = lib()
    buf = torch.zeros(64)  # 64-byte aligned host memory: never dereferenced by the calls below
    p, tab = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(torch.zeros(8, dtype=torch.int64).data_ptr())
    odd = ctypes.c_void_p(buf.data_ptr() + 4)
    count = L.rtfs_debug_launch_count()
    for Kmax in (0, 17, -1):
        assert L.rtfs_live_ingest_frame_faces_f32(tab, p, p, p, p, 1, 1, Kmax, 640, 1, 2560, 1280, 2560, None) == -4
        assert L.rtfs_live_overlap_add_faces_f32(tab, p, p, p, 1, 1280, Kmax, 2560, 1280, 2560, 0, None) == -4
    assert L.rtfs_live_ingest_frame_faces_f32(tab, p, p, p, p, 1, 1, 3, 640, 1, 2561, 1280, 2560, None) == -4  # window
    assert L.rtfs_live_overlap_add_faces_f32(tab, p, p, p, 1, 1280, 3, 2560, 1280, 641, 0, None) == -4  # max_chunk
    assert L.rtfs_live_ingest_frame_faces_f32(tab, p, odd, p, p, 1, 1, 3, 640, 1, 2560, 1280, 2560, None) == -4  # alignment
    assert L.rtfs_live_overlap_add_faces_f32(tab, odd, p, p, 1, 1280, 3, 2560, 1280, 2560, 0, None) == -4
    assert L.rtfs_live_ingest_frame_faces_f32(None, p, p, p, p, 1, 1, 3, 640, 1, 2560, 1280, 2560, None) == -4
    assert L.rtfs_live_ingest_frame_faces_f32(tab, p, p, p, p, 1, 1, 3, 2561, 1, 2560, 1280, 2560, None) != 0  # a chunk past max_chunk
    assert L.rtfs_live_ingest_frame_faces_f32(tab, p, p, p, p, 1, 0, 3, 0, 0, 2560, 1280, 2560, None) == 0  # the empty tick
    assert L.rtfs_live_overlap_add_faces_f32(tab, p, p, p, 1, 0, 3, 2560, 1280, 2560, 0, None) == 0
    assert L.rtfs_debug_launch_count() == count
