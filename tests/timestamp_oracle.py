"""The timestamp rule of DESIGN.md "Live streams with per-frame timestamps", by brute force with exact fractions.  Nothing here uses the
integer forms of csrc/frame_rate.h, imports the package under test or touches a device: seconds first, then ticks, then a search.

Camera frame i is stamped tau_i in a timebase of tb ticks per second, so it was taken at t_i = tau_i / tb seconds and its 25 fps tick is
r(i) = floor(25 t_i + 1/2).  Model frame p shows the last camera frame whose tick is at or before p and, before the first tick, the
first camera frame: c(p) = max(0, max{i : r(i) <= p}).  When every frame taken before the instant W / tb is in, the model frames
p < G(W) are final, G(W) = the number of ticks p with p + 1/2 <= 25 W / tb: a frame still to come is taken at W / tb or later, and its
tick lies at or before p exactly when 25 t + 1/2 < p + 1.

A stream (``Stream``) keeps n camera frames received, g model frames final, its last stamp and the watermark W:
  push(stamps, until):  refused unless the stamps increase, lie above the last stamp and at or above W;  W' = max(W, last stamp, until),
                        g' = max(g, G(W')), but 0 while no camera frame has ever arrived;  finalises g .. g' - 1
  flush(until):         g_end = max(g, G(max(W, until)), r(n - 1) + 1) (0 without a frame);  finalises g .. g_end - 1, then starts over
and reports for every newly final model frame the camera frame it shows, as a global index."""
import functools
from fractions import Fraction
from math import floor

MODEL_FPS = 25
MAX_TB, MAX_STAMP = 1 << 30, 1 << 40


class Refused(ValueError):
    pass


@functools.lru_cache(maxsize=None)
def tick(tau, tb):
    return floor(Fraction(tau, tb) * MODEL_FPS + Fraction(1, 2))


def final_count(W, tb):
    """G(W): walk the model frames while a frame taken at W / tb or later can no longer change them."""
    p, instant = 0, Fraction(W, tb) * MODEL_FPS
    while Fraction(p) + Fraction(1, 2) <= instant:
        p += 1
    return p


def source(p, stamps, tb):
    """c(p) over the frames ``stamps``: a linear search for the last one whose tick is at or before p; frame 0 when there is none."""
    best = 0
    for i, tau in enumerate(stamps):
        if tick(tau, tb) <= p:
            best = i
    return best


def end_count(stamps, tb, until=0):
    """The model frames of a whole track: the flush rule on a stream that has received everything and whose largest until is this."""
    if not stamps:
        return 0
    return max(final_count(max(stamps[-1], until), tb), tick(stamps[-1], tb) + 1)


def frame_map(stamps, tb, until=0):
    """[c(0), c(1), ...] of a whole track."""
    return [source(p, stamps, tb) for p in range(end_count(stamps, tb, until))]


class Stream:
    """One slot.  ``push`` / ``flush`` return the GLOBAL camera indices the newly final model frames show; ``clone`` gives a copy to try a
    call on.  ``max_final``: the most model frames one call may finalise (the pools' max_frames)."""

    def __init__(self, tb):
        if not 1 <= tb <= MAX_TB:
            raise Refused(f"timebase {tb}")
        self.tb, self.stamps, self.g, self.W = tb, [], 0, 0

    def clone(self):
        other = Stream(self.tb)
        other.stamps, other.g, other.W = list(self.stamps), self.g, self.W
        return other

    @property
    def n(self):
        return len(self.stamps)

    def check(self, stamps, until):
        prev = self.stamps[-1] if self.stamps else -1
        for tau in stamps:
            if not 0 <= tau < MAX_STAMP:
                raise Refused(f"stamp {tau}")
            if tau < self.W or tau <= prev:
                raise Refused(f"stamp {tau} behind {max(self.W, prev)}")
            prev = tau
        if not 0 <= until <= MAX_STAMP:
            raise Refused(f"until {until}")

    def push(self, stamps, until=0, max_final=None):
        self.check(stamps, until)
        W1 = max([self.W, until] + list(stamps[-1:]))
        allst = self.stamps + list(stamps)
        g1 = max(self.g, final_count(W1, self.tb)) if allst else 0
        if max_final is not None and g1 - self.g > max_final:
            raise Refused(f"{g1 - self.g} model frames in one push")
        new = [source(p, allst, self.tb) for p in range(self.g, g1)]
        self.stamps, self.g, self.W = allst, g1, W1
        return new

    def flush(self, until=0, max_final=None):
        self.check([], until)
        g1 = max(self.g, end_count(self.stamps, self.tb, max(self.W, until))) if self.stamps else 0
        if max_final is not None and g1 - self.g > max_final:
            raise Refused(f"{g1 - self.g} model frames in one flush")
        new = [source(p, self.stamps, self.tb) for p in range(self.g, g1)]
        self.stamps, self.g, self.W = [], 0, 0
        return new


def constant_rate(n, fin, tb):
    """The stamps of n frames at ``fin`` fps, tau_i = i tb / fin; the rates of the tests divide tb."""
    step = Fraction(tb) / Fraction(fin)
    assert step.denominator == 1, (fin, tb)
    return [i * int(step) for i in range(n)]
