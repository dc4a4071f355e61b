"""Numpy restatement (float64) of live streaming with faces that come and go (AVNet.open_streams(max_speakers=Kmax) / FaceStreamPool,
rtfs_live_faces_plan, rtfs_live_ingest_frame_faces_f32, rtfs_live_overlap_add_faces_f32), a thin layer on tests/live_oracle.py from the
rules of DESIGN.md "Faces that come and go".  Nothing here imports the package under test.

A slot keeps the four counters of one stream and a birth window per plane 0 .. Kmax - 1 (-1 = free).  A face added when the slot has
f frames is born at b = ceil(f / Hv); it takes part in window n iff n >= b; its output is the stream from sample b hop on, which is the
stream a recording cut at (b hop, b Hv) gives: ``OverlapAdd`` is live_oracle.OverlapAdd in coordinates shifted by b.  Counters,
readiness, the capacity rule and the slot's output range are live_oracle's, because a and f are shared."""
import numpy as np

from tests import live_oracle as VO
from tests import longform_oracle as LO

SPF, ALIGN = VO.SPF, VO.ALIGN
MAX_SPEAKERS, MAX_CAPACITY = 16, 1 << 24
BAD_ARGUMENT, UNKNOWN_SLOT, REPEATED_SLOT, CHUNK_SIZE, AUDIO_CAPACITY, VIDEO_CAPACITY, NO_FRAMES, BAD_COUNTERS, NO_FACES = range(1, 10)


class Refused(ValueError):
    def __init__(self, r, reason):
        super().__init__(f"index {r}: reason {reason}")
        self.r, self.reason = r, reason


def birth_at(f, hop):
    return -(-f // (hop // SPF))


def tick(counters, births, slot_ids, na, nf, window, hop, max_chunk, Kmax, flush=False, row_cap=1 << 30):
    """One push / flush of the named slots.  counters: dict slot -> (a, f, e, o); births: dict slot -> Kmax births; neither is modified.
    -> dict(new, rows = [(slot, n)], targets = [(slot, n, plane)] in target-row order, row_counts, ranges = [(o, end)] per named slot,
    face_ranges = per named slot {plane: (lo, end)} of the faces present, present = per named slot [(plane, birth)], off, floats,
    table = the (15 + 2 Kmax) R words of the C planner, sizes).  ``Refused`` carries the index and the reason the C planner reports."""
    try:
        VO.check_sizes(window, hop, max_chunk)
    except VO.Refused:
        raise Refused(-1, BAD_ARGUMENT) from None
    C, Hv, Wv = VO.capacity(window, max_chunk), hop // SPF, window // SPF
    if not 1 <= Kmax <= MAX_SPEAKERS or Kmax * C > MAX_CAPACITY or len(slot_ids) < 1:
        raise Refused(-1, BAD_ARGUMENT)
    for r, s in enumerate(slot_ids):
        if s not in counters:
            raise Refused(r, UNKNOWN_SLOT)
        if s in slot_ids[:r]:
            raise Refused(r, REPEATED_SLOT)
    new, rows, targets, row_counts, ranges, face_ranges, presents, off, floats, cols = dict(counters), [], [], [], [], [], [], [], 0, []
    max_span = max_na = max_nf = 0
    for r, s in enumerate(slot_ids):
        a, f, e, o = c = counters[s]
        if any(b < -1 or b > -(-f // Hv) for b in births[s]):
            raise Refused(r, BAD_COUNTERS)
        if flush:
            N = 0 if a == 0 else LO.plan(a, max(f, 1), window, hop)
            c1, wins, rng, sz = (0, 0, 0, 0), list(range(e, N)), (o, a), (0, 0)
            present = [(j, b) for j, b in enumerate(births[s]) if b >= 0 and N > b and f > b * Hv]
            if a > 0 and not present:
                raise Refused(r, NO_FRAMES)
            span = a - o
        else:
            if not 0 <= na[r] <= max_chunk or not 0 <= nf[r] <= max_chunk // SPF:
                raise Refused(r, CHUNK_SIZE)
            if a + na[r] - e * hop > C:
                raise Refused(r, AUDIO_CAPACITY)
            if f + nf[r] - e * Hv > C // SPF:
                raise Refused(r, VIDEO_CAPACITY)
            c1, wins, rng = VO.push_one(c, na[r], nf[r], window, hop, max_chunk)
            sz = (na[r], nf[r])
            present = [(j, b) for j, b in enumerate(births[s]) if b >= 0]
            if not present:
                raise Refused(r, NO_FACES)
            span = (c1[2] - 1) * hop + window - o if wins else 0
        if len(rows) + len(wins) > row_cap:
            raise Refused(r, BAD_ARGUMENT)
        P = len(present)
        cols.append([s, a, sz[0], f, sz[1], e, len(wins), len(rows), rng[0], rng[1], floats, a % C, f % (C // SPF), P, len(targets)] +
                    [j for j, _ in present] + [-1] * (Kmax - P) + [b for _, b in present] + [0] * (Kmax - P))
        new[s] = c1
        for n in wins:
            rows.append((s, n))
            here = [(s, n, j) for j, b in present if b <= n]
            targets += here
            row_counts.append(len(here))
        ranges.append(rng)
        face_ranges.append({j: (min(rng[1], max(rng[0], b * hop)), rng[1]) for j, b in present})
        presents.append(present)
        off.append(floats)
        floats += -(-P * (rng[1] - rng[0]) // ALIGN) * ALIGN
        max_span, max_na, max_nf = max(max_span, span), max(max_na, sz[0]), max(max_nf, sz[1])
    table = [col[k] for k in range(15 + 2 * Kmax) for col in cols]
    return dict(new=new, rows=rows, targets=targets, row_counts=row_counts, ranges=ranges, face_ranges=face_ranges, present=presents, off=off,
                floats=floats, table=table, sizes=[len(rows), len(targets), floats, max_span, max_na, max_nf])


def frame_rows(rows, targets, hist, limits, window, hop):
    """The framed windows of one tick.  hist: slot -> (x (a',), {plane: v (512, f')}) in STREAM coordinates (a face's columns before its
    first frame are never read); limits: slot -> (L, Tv).  -> xw (rows, window), once per window, and vw (targets, 512, window / 640) at
    the ragged target rows: live_oracle.frame_rows per target."""
    xw = VO.frame_rows(rows, {s: (x, next(iter(v.values()))) for s, (x, v) in hist.items()}, limits, window, hop)[0]
    vw = np.zeros((len(targets), 512, window // SPF), np.float32)
    for t, (s, n, j) in enumerate(targets):
        vw[t] = VO.frame_rows([(s, n)], {s: (hist[s][0], hist[s][1][j])}, limits, window, hop)[1][0]
    return xw, vw


class OverlapAdd:
    """The streaming overlap-add of ONE face born at window ``birth``: live_oracle.OverlapAdd of the stream that starts at birth * hop."""

    def __init__(self, window, hop, birth):
        self.hop, self.birth, self.ola = hop, birth, VO.OverlapAdd(window, hop, 1)

    def feed(self, n, y):
        self.ola.feed(n - self.birth, np.asarray(y)[None])

    def take(self, lo, end):
        """Samples [lo, end) of the SLOT's stream, lo >= birth * hop."""
        s = self.birth * self.hop
        assert lo >= s or lo >= end
        return self.ola.take(lo - s, end - s)[0] if end > lo else np.zeros(0)


def continue_schedule(c, L, Tv, sizes, window, hop, max_chunk, start=0):
    """live_oracle.schedule in mode "step" from counters ``c`` on: [(na, nf)] that deliver the rest of L samples and Tv frames."""
    cap_f, out, i = max_chunk // SPF, [], start
    while c[0] < L or c[1] < Tv:
        na = min(min(sizes[i % len(sizes)], max_chunk), L - c[0])
        i += 1
        want = Tv if c[0] + na == L else (c[0] + na) // SPF
        nf = min(max(min(want, Tv) - c[1], 0), cap_f)
        for trial in ((na, nf), (0, min(cap_f, Tv - c[1])), (min(max_chunk, L - c[0]), 0), (0, 1), (1, 0)):
            try:
                c1 = VO.push_one(c, trial[0], trial[1], window, hop, max_chunk)[0]
            except VO.Refused:
                continue
            if c1 != c or trial == (na, nf):
                break
        else:
            raise AssertionError(f"stuck at {c}")
        out.append(trial)
        c = c1
    return out


def merge(scripts):
    """Per-slot scripts -> events.  A script is a list of steps: ("add", plane or None), ("drop", plane), ("push", na, nf); tick i holds
    the i-th push of every slot that still has one, with the adds / drops in front of it first, and a slot is flushed in the tick after
    its last push (adds / drops behind the last push come before the flush)."""
    per = {}
    for s, steps in scripts.items():
        ticks, pre = [], []
        for st in steps:
            if st[0] == "push":
                ticks.append((pre, st[1], st[2]))
                pre = []
            else:
                pre.append(st)
        per[s] = (ticks, pre)
    ev = []
    for i in range(max(len(t) for t, _ in per.values()) + 1):
        done = [s for s, (t, _) in per.items() if len(t) == i]
        for s in done:
            ev += [(kind, s, j) for kind, j in per[s][1]]
        if done:
            ev.append(("flush", done, None, None))
        ids = [s for s, (t, _) in per.items() if len(t) > i]
        for s in ids:
            ev += [(kind, s, j) for kind, j in per[s][0][i][0]]
        if ids:
            ev.append(("push", ids, [per[s][0][i][1] for s in ids], [per[s][0][i][2] for s in ids]))
    return ev


def random_scripts(rng, slots, Kmax, window, hop, max_chunk, pushes):
    """Seeded random per-slot scripts with joins and drops; every push is one the capacity rule accepts."""
    C, Hv = VO.capacity(window, max_chunk), hop // SPF
    sizes = VO.chunk_sizes(hop, max_chunk) + [window, 2 * hop]
    scripts = {}
    for s in range(slots):
        c, active, steps = (0, 0, 0, 0), set(), []
        for _ in range(int(rng.randint(1, pushes + 1))):
            for _ in range(3):
                free = [j for j in range(Kmax) if j not in active]
                u = rng.rand()
                if free and (not active or u < 0.25):
                    j = free[int(rng.randint(len(free)))] if rng.rand() < 0.5 else None
                    active.add(min(free) if j is None else j)
                    steps.append(("add", j))
                elif len(active) > 1 and u > 0.8:
                    j = sorted(active)[int(rng.randint(len(active)))]
                    active.discard(j)
                    steps.append(("drop", j))
            na = min(int(sizes[int(rng.randint(len(sizes)))]), max_chunk)
            nf = int(rng.randint(0, max_chunk // SPF + 1)) if rng.rand() < 0.3 else max(0, min((c[0] + na) // SPF - c[1], max_chunk // SPF))
            for trial in ((na, nf), (0, nf), (na, 0), (0, 0)):
                try:
                    c = VO.push_one(c, trial[0], trial[1], window, hop, max_chunk)[0]
                    break
                except VO.Refused:
                    continue
            steps.append(("push",) + trial)
        if c[0] > 0 and c[1] == 0:  # a stream with samples needs a frame before its flush
            steps.append(("push", 0, 1))
        scripts[s] = steps
    assert C > 0 and Hv > 0
    return scripts
