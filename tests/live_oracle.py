"""Numpy restatement (float64) of live streaming (AVNet.open_streams / StreamPool, rtfs_live_*), from the rules of DESIGN.md "Live
streams".  Nothing here imports the package under test; the only thing shared with tests/longform_oracle.py is the weight formula.

A stream has four counters: a samples received, f frames received, e windows emitted, o samples output.  With Wv = window / 640 and
Hv = hop / 640, window n is ready when a >= n hop + window and f >= n Hv + Wv.  A push adds its chunks, emits every ready window
n = e, e + 1, ... and makes [o, e_new hop) final.  A flush takes L = a, Tv = f, emits the windows the long-form plan still owes (N = 1 if
L <= window else 1 + ceil((L - window) / hop)) and makes [o, L) final, then zeroes the counters.  The history ring of a slot holds
C = window + max_chunk samples (C / 640 frames); a push is refused when a + na - e hop > C or f + nf - e Hv > C / 640, because the
chunk would then land on a cell that window e still needs."""
import numpy as np

from tests import longform_oracle as LO

SPF = 640
ALIGN = 32


class Refused(ValueError):
    pass


def capacity(window, max_chunk):
    return window + max_chunk


def check_sizes(window, hop, max_chunk):
    if window <= 0 or window % SPF or hop % SPF or not 0 < hop <= window or max_chunk < SPF or max_chunk % SPF:
        raise Refused(f"window {window} hop {hop} max_chunk {max_chunk}")


def push_one(c, na, nf, window, hop, max_chunk):
    """counters (a, f, e, o) and the sizes of one push -> new counters, [window indices], (o, end).  Refused when the formulas forbid it."""
    a, f, e, o = c
    C, Hv, Wv = capacity(window, max_chunk), hop // SPF, window // SPF
    if not 0 <= na <= max_chunk or not 0 <= nf <= max_chunk // SPF:
        raise Refused(f"chunk of {na} samples / {nf} frames")
    if a + na - e * hop > C or f + nf - e * Hv > C // SPF:
        raise Refused("capacity")
    a, f = a + na, f + nf
    wins = []
    while a >= (e + len(wins)) * hop + window and f >= (e + len(wins)) * Hv + Wv:
        wins.append(e + len(wins))
    e1 = e + len(wins)
    return (a, f, e1, e1 * hop), wins, (o, e1 * hop)


def flush_one(c, window, hop):
    a, f, e, o = c
    if a == 0:
        return (0, 0, 0, 0), [], (o, o)
    if f < 1:
        raise Refused("samples but no frame")
    N = LO.plan(a, f, window, hop)
    return (0, 0, 0, 0), list(range(e, N)), (o, a)


def tick(counters, slot_ids, na, nf, window, hop, max_chunk, n_src=1, flush=False):
    """One push / flush of the named slots on ``counters`` (dict slot -> (a, f, e, o), NOT modified): -> dict(new = counters after,
    rows = [(slot, n)] in the order the slots are named then by window index, ranges = [(o, end)] per named slot, off = start of each
    slot's (n_src, end - o) block in the flat output, floats = its size, table = the 13 columns the C planner writes)."""
    check_sizes(window, hop, max_chunk)
    if len(set(slot_ids)) != len(slot_ids) or any(s not in counters for s in slot_ids):
        raise Refused(f"slot ids {slot_ids}")
    C = capacity(window, max_chunk)
    new, rows, ranges, off, floats, cols = dict(counters), [], [], [], 0, []
    for r, s in enumerate(slot_ids):
        c = counters[s]
        if flush:
            c1, wins, rng = flush_one(c, window, hop)
            sizes = (0, 0)
        else:
            c1, wins, rng = push_one(c, na[r], nf[r], window, hop, max_chunk)
            sizes = (na[r], nf[r])
        cols.append([s, c[0], sizes[0], c[1], sizes[1], c[2], len(wins), len(rows), rng[0], rng[1], floats, c[0] % C, c[1] % (C // SPF)])
        new[s] = c1
        rows += [(s, n) for n in wins]
        ranges.append(rng)
        off.append(floats)
        floats += -(-n_src * (rng[1] - rng[0]) // ALIGN) * ALIGN
    table = [col[k] for k in range(13) for col in cols]
    return dict(new=new, rows=rows, ranges=ranges, off=off, floats=floats, table=table)


def frame_rows(rows, hist, limits, window, hop):
    """The framed windows of one tick.  hist: slot -> (x (a',) , v (512, f')) = everything the slot has received INCLUDING this push;
    limits: slot -> (L, Tv) = (a', f').  Window n = samples [n hop, n hop + window) with zeros past L and frames n Hv + j with an index
    past Tv - 1 reading frame Tv - 1.  Copies: the dtype is kept."""
    Wv = window // SPF
    xw = np.zeros((len(rows), window), np.float32)
    vw = np.zeros((len(rows), 512, Wv), np.float32)
    for i, (s, n) in enumerate(rows):
        x, v = hist[s]
        L, Tv = limits[s]
        seg = x[n * hop:min(L, n * hop + window)]
        xw[i, :seg.shape[0]] = seg
        vw[i] = v[:, np.minimum(n * hop // SPF + np.arange(Wv), Tv - 1)]
    return xw, vw


class OverlapAdd:
    """Streaming overlap-add of ONE stream in float64.  feed(n, y_n) in ascending n adds w * y_n; take(o, end) returns samples [o, end)
    divided by the weights of the windows fed SO FAR.  That these are already the final weights for a sample below e hop is what
    tests/test_live_host.py checks against longform_oracle.overlap_add of the whole recording."""

    def __init__(self, window, hop, n_src):
        self.window, self.hop, self.w = window, hop, LO.weights(window, hop)
        self.num, self.den, self.next = np.zeros((n_src, 0)), np.zeros(0), 0

    def feed(self, n, y):
        assert n == self.next, (n, self.next)
        self.next += 1
        need = n * self.hop + self.window
        if need > self.den.shape[0]:
            self.num = np.concatenate([self.num, np.zeros((self.num.shape[0], need - self.den.shape[0]))], axis=1)
            self.den = np.concatenate([self.den, np.zeros(need - self.den.shape[0])])
        self.num[:, n * self.hop:need] += self.w * np.asarray(y, np.float64)
        self.den[n * self.hop:need] += self.w

    def take(self, o, end):
        return self.num[:, o:end] / self.den[o:end]


# ---------------------------------------------------------------- schedules: ways of cutting one recording into pushes
def chunk_sizes(hop, max_chunk):
    return [0, 1, 639, 640, 641, hop - 1, hop, hop + 1, max_chunk]


def schedule(L, Tv, sizes, mode, window, hop, max_chunk, start=0):
    """A list of (na, nf) that delivers L samples and Tv frames.  Audio chunk sizes cycle through ``sizes`` from ``start``; video follows
    ``mode``: "step" (the frames complete so far), "lag" (a window behind), "lead" (a window ahead).  A push the capacity rule would
    refuse is replaced by one that only lets the side that is behind catch up."""
    cap_f, lagf = max_chunk // SPF, window // SPF
    c, out, i = (0, 0, 0, 0), [], start
    while c[0] < L or c[1] < Tv:
        na = min(min(sizes[i % len(sizes)], max_chunk), L - c[0])
        i += 1
        want = (c[0] + na) // SPF + {"step": 0, "lag": -lagf, "lead": lagf}[mode]
        if c[0] + na == L:
            want = Tv
        nf = min(max(min(want, Tv) - c[1], 0), cap_f)
        for trial in ((na, nf), (0, min(cap_f, Tv - c[1])), (min(max_chunk, L - c[0]), 0), (0, 1), (1, 0)):
            try:
                c1 = push_one(c, trial[0], trial[1], window, hop, max_chunk)[0]
            except Refused:
                continue
            if c1 != c or trial == (na, nf):
                break
        else:
            raise AssertionError(f"stuck at {c}")
        out.append(trial)
        c = c1
    return out


def events(schedules):
    """Per-slot schedules -> [("push", ids, na, nf)] with push i of every slot that still has one in tick i, then ("flush", [slot]) in the
    tick after a slot's last push."""
    ev, n = [], max(len(s) for s in schedules.values())
    for i in range(n + 1):
        done = [s for s, sch in schedules.items() if len(sch) == i]
        if done:
            ev.append(("flush", done, None, None))
        ids = [s for s, sch in schedules.items() if len(sch) > i]
        if ids:
            ev.append(("push", ids, [schedules[s][i][0] for s in ids], [schedules[s][i][1] for s in ids]))
    return ev
