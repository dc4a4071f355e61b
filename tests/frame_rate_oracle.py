"""The frame-rate rule of DESIGN.md "Live streams at the camera's frame rate", by brute force with exact fractions.  Nothing here uses
the closed forms of csrc/frame_rate.h: ticks first, then a search.

Camera frame i of a stream at ``fin`` fps has the 25 fps tick r(i) = floor(i 25 / fin + 1/2).  Model frame p shows the last camera frame
whose tick is at or before p, c(p) = max{i : r(i) <= p}.  A stream that has received n camera frames has exactly the model frames p
with c(p) < n."""
import functools
from fractions import Fraction
from math import floor

MODEL_FPS = 25
# the rates of the host tests (tests/test_frame_rate_host.py)
RATES = [Fraction(30), Fraction(60), Fraction(50), Fraction(24), Fraction(15), Fraction(10), Fraction(25, 2), Fraction(30000, 1001),
         Fraction(25)]


@functools.lru_cache(maxsize=None)
def tick(i, fin):
    return floor(Fraction(i) * MODEL_FPS / Fraction(fin) + Fraction(1, 2))


def source(p, fin):
    """c(p): walk the camera frames until the first whose tick lies behind p (ticks never decrease)."""
    assert tick(0, fin) == 0
    i = 0
    while tick(i + 1, fin) <= p:
        i += 1
    return i


def frame_map(n, fin):
    """The camera frames that the model frames of a stream of n camera frames show, in order: [c(0), c(1), ...] while c(p) < n.  The
    walk of ``source`` carried on from frame to frame."""
    out, p, i = [], 0, 0
    while n > 0:
        while tick(i + 1, fin) <= p:
            i += 1
        if i >= n:
            break
        out.append(i)
        p += 1
    return out


def count(n, fin):
    return len(frame_map(n, fin))


def push_selection(n0, mc, fin):
    """What a push of mc camera frames to a stream that had received n0 adds: the LOCAL indices (into the chunk) of the model frames
    P(n0) .. P(n0 + mc) - 1."""
    full = frame_map(n0 + mc, fin)
    new = full[count(n0, fin):]
    assert all(n0 <= c < n0 + mc for c in new), (n0, mc, fin, new)  # consequence 1: a new model frame always shows a frame of this chunk
    return [c - n0 for c in new]
