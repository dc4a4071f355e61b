"""Numpy restatement of live streams from camera frames (FRCNNVideoModel.open_streams / LipStreamPool, System.open_camera_streams /
CameraStreamPool, rtfs_live_video_*), from the rules of DESIGN.md "Live streams from camera frames".  Nothing here imports the package
under test or touches a device.

A lip track has two counters: g frames received, v embeddings emitted (the planner carries a third word, the side of the history that
is current: it flips with every push that brings a frame).  The front-end's stem is a Conv3d with temporal kernel 5 and padding 2 and
everything behind it works frame by frame, so embedding q is the front-end applied to the prepared lips frames q - 2 .. q + 2.
  push of m frames (0 <= m <= max_frames): g' = g + m, v' = max(v, g' - 2); emits v .. v' - 1.  Frames with index < 0 are zero planes.
  flush: emits v .. g - 1 with zero planes for indices >= g, then resets the slot.
Zero planes are 0.0f in the PREPARED domain (the stem's own padding), not f(0) of a black uint8 frame; the 3-pixel border of every plane
is zero as well.  uint8 ROIs go through the "val" chain: centre crop 88 x 88, f(v) = (float)(((double(v) - 0.0) / 255.0 - mean) / std)."""
import numpy as np

from tests import live_oracle as VO

ALIGN = 32
MEAN, STD = 0.421, 0.165  # transform.py:151-167
SIZES = (0, 1, 2, 3, 4, 5, 7)  # + max_frames: what the chunk-size cycles are drawn from


class Refused(ValueError):
    pass


def push_one(c, m, max_frames):
    """(g, v) and a chunk of m frames -> new (g, v), (first, end) of the embeddings emitted."""
    g, v = c
    if not 0 <= m <= max_frames:
        raise Refused(f"chunk of {m} frames")
    g1 = g + m
    v1 = max(v, g1 - 2)
    return (g1, v1), (v, v1)


def flush_one(c):
    g, v = c
    return (0, 0), (v, g)


def reads(q, limit):
    """The frames embedding q reads when `limit` frames exist: q - 2 .. q + 2 clipped to [0, limit)."""
    return [p for p in range(q - 2, q + 3) if 0 <= p < limit]


def tick(counters, slot_ids, ms, max_frames, flush=False):
    """One push / flush of the named slots on ``counters`` (dict slot -> (g, v, side), NOT modified): -> dict(new, rows = [(slot, q)] in the
    order the slots are named then by frame index, ranges = [(first, end)] per named slot, off, floats, table = the 8 columns of the C
    planner, max_m)."""
    if len(set(slot_ids)) != len(slot_ids) or any(s not in counters for s in slot_ids) or not slot_ids or max_frames < 1:
        raise Refused(f"slot ids {slot_ids}")
    new, rows, ranges, off, floats, cols = dict(counters), [], [], [], 0, []
    for r, s in enumerate(slot_ids):
        g, v, side = counters[s]
        if g < 0 or v < 0 or v > g or v < max(0, g - 2) or side not in (0, 1):
            raise Refused(f"counters {counters[s]}")
        if flush:
            (g1, v1), rng = flush_one((g, v))
            m, side1 = 0, 0
        else:
            m = ms[r]
            (g1, v1), rng = push_one((g, v), m, max_frames)
            side1 = 1 - side if m > 0 else side
        cols.append([s, g, m, v, rng[1] - rng[0], len(rows), floats, side])
        new[s] = (g1, v1, side1)
        rows += [(s, q) for q in range(*rng)]
        ranges.append(rng)
        off.append(floats)
        floats += -(-512 * (rng[1] - rng[0]) // ALIGN) * ALIGN
    table = [col[k] for k in range(8) for col in cols]
    return dict(new=new, rows=rows, ranges=ranges, off=off, floats=floats, table=table, max_m=max([0] if flush else list(ms)))


def center_offsets(H, W):
    return int(round((H - 88)) / 2.0), int(round((W - 88)) / 2.0)  # the reference's rounding: an odd difference truncates


def prepare_u8(roi):
    """uint8 (n, H, W) -> float32 prepared lips (n, 88, 88) by the "val" chain."""
    dy, dx = center_offsets(roi.shape[1], roi.shape[2])
    lut = (((np.arange(256, dtype=np.float64) - 0.0) / 255.0 - MEAN) / STD).astype(np.float32)
    return lut[roi[:, dy:dy + 88, dx:dx + 88]]


def windows(rows, hist, limits):
    """The stem input of one tick, (len(rows), 5, 94, 94): for row (s, q) the prepared frames q - 2 .. q + 2 of hist[s] (everything slot s
    has received INCLUDING this push, (n, 88, 88) float32) inside a zero border of 3 pixels; a frame index < 0 or >= limits[s] is a zero
    plane.  Copies: the bits are kept."""
    out = np.zeros((len(rows), 5, 94, 94), np.float32)
    for i, (s, q) in enumerate(rows):
        for j in range(5):
            p = q - 2 + j
            if 0 <= p < limits[s]:
                out[i, j, 3:91, 3:91] = hist[s][p]
    return out


def history(frames, g):
    """What the slot's current history buffer must hold after g frames: {plane p % 4: frame p} for p in [max(0, g - 4), g)."""
    return {p % 4: frames[p] for p in range(max(0, g - 4), g)}


def chunking(Tv, sizes, start=0):
    """Chunk sizes that deliver Tv frames, cycling through ``sizes`` from ``start`` (zeros stay in: an empty push is a push)."""
    out, i, g = [], start, 0
    while g < Tv:
        m = min(sizes[i % len(sizes)], Tv - g)
        i += 1
        out.append(m)
        g += m
    return out


def events(schedules):
    """Per-slot lists of chunk sizes -> [("push", ids, ms)] with push i of every slot that still has one in tick i, then ("flush", ids) in
    the tick after a slot's last push."""
    ev, n = [], max(len(s) for s in schedules.values())
    for i in range(n + 1):
        done = [s for s, sch in schedules.items() if len(sch) == i]
        if done:
            ev.append(("flush", done, None))
        ids = [s for s, sch in schedules.items() if len(sch) > i]
        if ids:
            ev.append(("push", ids, [schedules[s][i] for s in ids]))
    return ev


# ---------------------------------------------------------------- the camera pool: a lip stream in front of tests/live_oracle.py
SLACK = 2 * VO.SPF  # the inner audio pool is opened with max_chunk + 1280: embeddings lag the frames received by two frames


def camera_push(ca, cv, na, m, window, hop, max_chunk, inner_chunk):
    """Audio counters ca = (a, f, e, o) of the inner pool and lip counters cv = (g, v): a push of na samples and m frames.  The outer pool
    takes chunks up to max_chunk samples / max_chunk // 640 frames and frames up to (window + max_chunk) / 640 + 2 ahead of the first
    window not yet emitted (so that the two embeddings a flush still owes always fit); the k embeddings the lip push emits are the inner
    pool's video chunk, and the inner pool (capacity window + inner_chunk) refuses as tests/live_oracle.py says."""
    if not 0 <= na <= max_chunk:
        raise VO.Refused(f"chunk of {na} samples")
    try:
        cv1, (v0, v1) = push_one(cv, m, max_chunk // VO.SPF)
    except Refused as e:
        raise VO.Refused(str(e)) from None
    if cv1[0] - ca[2] * (hop // VO.SPF) > (window + max_chunk) // VO.SPF + 2:
        raise VO.Refused("capacity (frames)")
    ca1, wins, rng = VO.push_one(ca, na, v1 - v0, window, hop, inner_chunk)
    return ca1, cv1, wins, rng


def camera_flush(ca, cv, window, hop, inner_chunk):
    """Lip flush, its k <= 2 embeddings pushed with empty audio, inner flush -> ((0,) * 4, (0, 0), windows, (o, L))."""
    _, (v0, g) = flush_one(cv)
    ca1, wins, (o, _) = VO.push_one(ca, 0, g - v0, window, hop, inner_chunk)
    ca2, wins2, (_, end) = VO.flush_one(ca1, window, hop)
    return ca2, (0, 0), wins + wins2, (o, end)


def in_step(L, sizes, max_chunk, start=0):
    """Audio chunk sizes cycle through ``sizes``; every push brings the frames complete so far, (a + na) // 640 - g, and the last one the
    rest of Tv = ceil(L / 640).  No push is ever replaced."""
    out, a, g, i, Tv = [], 0, 0, start, -(-L // VO.SPF)
    while a < L:
        na = min(sizes[i % len(sizes)], max_chunk, L - a)
        i += 1
        a += na
        nf = (Tv if a == L else a // VO.SPF) - g
        g += nf
        out.append((na, nf))
    return out


def camera_schedule(L, Tv, sizes, mode, window, hop, max_chunk, inner_chunk, start=0):
    """tests/live_oracle.schedule for the camera pool: a push the pool would refuse is replaced by one that lets the side that is behind
    catch up.  -> [(na, nf, replaced)]."""
    cap_f, lagf = max_chunk // VO.SPF, window // VO.SPF
    ca, cv, out, i = (0, 0, 0, 0), (0, 0), [], start
    while ca[0] < L or cv[0] < Tv:
        na = min(min(sizes[i % len(sizes)], max_chunk), L - ca[0])
        i += 1
        want = (ca[0] + na) // VO.SPF + {"step": 0, "lag": -lagf, "lead": lagf}[mode]
        if ca[0] + na == L:
            want = Tv
        nf = min(max(min(want, Tv) - cv[0], 0), cap_f)
        for trial in ((na, nf), (0, min(cap_f, Tv - cv[0])), (min(max_chunk, L - ca[0]), 0), (0, 1), (1, 0)):
            try:
                ca1, cv1, _, _ = camera_push(ca, cv, trial[0], trial[1], window, hop, max_chunk, inner_chunk)
            except VO.Refused:
                continue
            if (ca1, cv1) != (ca, cv) or trial == (na, nf):
                break
        else:
            raise AssertionError(f"stuck at {ca} {cv}")
        out.append((trial[0], trial[1], trial != (na, nf)))
        ca, cv = ca1, cv1
    return out
