"""Numpy restatement of live streams at the microphone's rate (datas.open_resample_streams / ResampleStreamPool, the ``sample_rate``
keyword of the open_* entries / RateStreamPool, rtfs_live_resample_*), from the rules of DESIGN.md "Live streams at the microphone's
rate".  Nothing here imports the package under test or touches a device.

In the notation of tests/prep_oracle.resample_plan (o, n, width; c(p) = floor(o p / n)) output q = j n + p of a recording reads the inputs
first(q) = j o + c(p) - width .. last(q) = j o + c(p) + width.  A stream has two counters: a input samples received, g outputs emitted
(the planner carries a third word, the side of the history that is current: it flips with every push that brings a sample).
  push of m samples (0 <= m <= max_chunk): a' = a + m, g' = G(a') = #{q : last(q) < a'}; emits g .. g' - 1.
  flush: emits g .. ceil(n a / o) - 1 with zeros for input indices >= a, then resets the slot.
G is COUNTED here (a sorted table of last(q)); that it is ceil(n max(0, A - width) / o) is the C planner's business.  The expected
outputs are slices of tests/prep_oracle.resample of the whole recording."""
import numpy as np

from tests import live_oracle as VO
from tests import live_video_oracle as LV
from tests import prep_oracle as PO

ALIGN = 32
RATIOS = [(3, 1), (2, 1), (1, 2), (1, 3), (441, 160), (441, 320), (441, 640)]  # reduced orig : new

chunking, events = LV.chunking, LV.events  # chunk sizes that deliver a length; per-slot size lists -> push / flush events


class Refused(ValueError):
    pass


class Plan:
    """o, n, width of a ratio and last(q) for the first `reach` input samples' worth of outputs."""

    def __init__(self, orig, new, reach=0):
        self.o, self.n, self.width, self.taps = PO.resample_plan(orig, new)
        self.orig, self.new = orig, new
        self._lasts = np.zeros(0, np.int64)
        self.extend(reach)

    def extend(self, reach):
        """Tabulate last(q) for every q with last(q) < reach (and some more)."""
        frames = reach // self.o + 2
        if frames * self.n > self._lasts.shape[0]:
            q = np.arange(frames * self.n, dtype=np.int64)
            self._lasts = (q // self.n) * self.o + (self.o * (q % self.n)) // self.n + self.width
            assert np.all(np.diff(self._lasts) >= 0)  # last(q) never decreases: the emitted outputs are a prefix

    def first(self, q):
        return (q // self.n) * self.o + (self.o * (q % self.n)) // self.n - self.width

    def last(self, q):
        return self.first(q) + 2 * self.width

    def G(self, A):
        """#{q : last(q) < A}, counted."""
        self.extend(A)
        return int(np.searchsorted(self._lasts, A, side="left"))

    def out_len(self, L):
        return -(-self.n * L // self.o)

    def tail(self):
        """The most a flush can emit (the bound the open_* entries hold against max_chunk)."""
        return -(-self.n * self.width // self.o) + 1


def push_one(P, c, m, max_chunk):
    """(a, g) and a chunk of m samples -> new (a, g), (first, end) of the outputs emitted."""
    a, g = c
    if not 0 <= m <= max_chunk:
        raise Refused(f"chunk of {m} samples")
    g1 = P.G(a + m)
    return (a + m, g1), (g, g1)


def flush_one(P, c):
    a, g = c
    return (0, 0), (g, P.out_len(a))


def tick(P, counters, slot_ids, ms, max_chunk, flush=False):
    """One push / flush of the named slots on ``counters`` (dict slot -> (a, g, side), NOT modified): -> dict(new, ranges = [(first, end)]
    per named slot, off, floats, table = the 7 columns of the C planner, max_m, max_k)."""
    if len(set(slot_ids)) != len(slot_ids) or any(s not in counters for s in slot_ids) or not slot_ids or max_chunk < 1:
        raise Refused(f"slot ids {slot_ids}")
    new, ranges, off, floats, cols = dict(counters), [], [], 0, []
    for r, s in enumerate(slot_ids):
        a, g, side = counters[s]
        if a < 0 or g != P.G(a) or side not in (0, 1):
            raise Refused(f"counters {counters[s]}")
        if flush:
            (a1, g1), rng = flush_one(P, (a, g))
            m, side1 = 0, 0
        else:
            m = ms[r]
            (a1, g1), rng = push_one(P, (a, g), m, max_chunk)
            side1 = 1 - side if m > 0 else side
        cols.append([s, a, m, g, rng[1] - rng[0], floats, side])
        new[s] = (a1, g1, side1)
        ranges.append(rng)
        off.append(floats)
        floats += -(-(rng[1] - rng[0]) // ALIGN) * ALIGN
    table = [col[k] for k in range(7) for col in cols]
    return dict(new=new, ranges=ranges, off=off, floats=floats, table=table, max_m=max([0] if flush else list(ms)),
                max_k=max(hi - lo for lo, hi in ranges))


def history(P, x, a):
    """What the slot's current history buffer must hold after a samples: {cell: sample} for the inputs max(0, a - 2 width) .. a - 1, input
    i in cell i - (a - 2 width)."""
    H = 2 * P.width
    return {i - (a - H): x[i] for i in range(max(0, a - H), a)}


def pcm(x):
    """float samples in [-1, 1) -> int16 PCM and the float32 values it stands for, s / 32768 (exact)."""
    s = np.clip(np.round(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    return s, (s.astype(np.float32) / np.float32(32768.0))


def sizes(P, max_chunk):
    """What the chunk-size cycles are drawn from: the history is refilled partly, exactly and wholly from a chunk."""
    w = P.width
    return sorted({0, 1, 2, w, 2 * w - 1, 2 * w, 2 * w + 1, max(P.o - 1, 0), P.o + 1, max_chunk})


def lengths(P):
    w = P.width
    return sorted({1, 2 * w - 1, 2 * w, 2 * w + 1, max(P.o - 1, 1), P.o, P.o + 1})


# ---------------------------------------------------------------- the composite pools: a resampler in front of tests/live_oracle.py
ROOM = VO.SPF  # the inner pool is opened with max_chunk + 640: a chunk of floor(max_chunk o / n) samples can give max_chunk + 1 outputs


def rate_push(P, cr, ca, cv, m, nf, window, hop, max_chunk, camera):
    """Resampler counters cr = (a, g), inner audio counters ca = (a, f, e, o) and, for the camera pool, lip counters cv = (g, v): a push of
    m input samples and nf frames (camera) / embeddings.  The k outputs the resampler emits are the inner pool's audio chunk; the inner
    pool was opened with max_chunk + 640; and the push is refused unless the resampler's flush tail still fits the inner ring behind it."""
    cr1, (g0, g1) = push_one(P, cr, m, max_chunk * P.o // P.n)
    if not 0 <= nf <= max_chunk // VO.SPF:
        raise VO.Refused(f"chunk of {nf} frames")
    if camera:
        inner = max_chunk + ROOM + LV.SLACK
        ca1, cv1, wins, rng = LV.camera_push(ca, cv, g1 - g0, nf, window, hop, max_chunk + ROOM, inner)
    else:
        inner = max_chunk + ROOM
        (ca1, wins, rng), cv1 = VO.push_one(ca, g1 - g0, nf, window, hop, inner), cv
    if ca1[0] + P.tail() - ca1[2] * hop > window + inner:
        raise VO.Refused("capacity (the flush tail)")
    return cr1, ca1, cv1, wins, rng


def rate_schedule(P, L, Tv, in_sizes, mode, window, hop, max_chunk, camera, start=0):
    """tests/live_oracle.schedule for the composite pools, L in INPUT samples: a push the pool would refuse is replaced by one that lets
    the side that is behind catch up.  -> [(m, nf)]."""
    cap_f, lagf, cap_in = max_chunk // VO.SPF, window // VO.SPF, max_chunk * P.o // P.n
    cr, ca, cv, out, i = (0, 0), (0, 0, 0, 0), (0, 0), [], start
    got = lambda: cv[0] if camera else ca[1]  # noqa: E731  frames delivered
    while cr[0] < L or got() < Tv:
        m = min(min(in_sizes[i % len(in_sizes)], cap_in), L - cr[0])
        i += 1
        want = P.out_len(cr[0] + m) // VO.SPF + {"step": 0, "lag": -lagf, "lead": lagf}[mode]
        if cr[0] + m == L:
            want = Tv
        nf = min(max(min(want, Tv) - got(), 0), cap_f)
        for trial in ((m, nf), (0, min(cap_f, Tv - got())), (min(cap_in, L - cr[0]), 0), (0, 1), (min(1, L - cr[0]), 0)):
            try:
                cr1, ca1, cv1, _, _ = rate_push(P, cr, ca, cv, trial[0], trial[1], window, hop, max_chunk, camera)
            except (VO.Refused, Refused):
                continue
            if (cr1, ca1, cv1) != (cr, ca, cv) or trial == (m, nf):
                break
        else:
            raise AssertionError(f"stuck at {cr} {ca} {cv}")
        out.append(trial)
        cr, ca, cv = cr1, ca1, cv1
    return out
