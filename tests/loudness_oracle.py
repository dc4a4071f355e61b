"""ITU-R BS.1770 integrated loudness as the library defines it (include/rtfs_amd.h "Loudness"; DESIGN.md "Loudness"), restated.

* ``design``            the filter design formulas, float64
* ``truth``             the plain sample recurrence of the two biquads in ``np.longdouble`` (80-bit on x86): hop energies and block
                        energies z of a set of recordings, the recordings side by side in one vector so that the sample loop runs once
* ``plain64``           the same plain recurrence in float64
* ``device64``          the device's own formulation in float64: a hop cut into 64 pieces run from zero state, piece ends combined
                        with A^p, hop ends combined with A^H, a second sweep from the true states, the lanes summed by butterfly
* ``gate``              both gates in the z domain -> (lufs, kept)
* ``assert_gate_margin``  no block of a test input may lie within 1e-6 relative of either threshold in ``truth``
* ``gpu_cases``         the seeded inputs of tests/test_hip_loudness.py

THE BAR.  ``measure()`` gives the worst relative deviation from ``truth`` of the two float64 restatements over ``gpu_cases()``, for
the block energies z of every block and for the hop energies of every hop whose mean square lies above the absolute gate (a hop
inside a stretch of exact zeros holds 10^-20 of the signal's energy and less; it is compared through its blocks only).
Measured with x86-64 80-bit long double as the reference, rounded up:
    plain64   z 5.2e-12   hops 7.0e-14
    device64  z 3.0e-12   hops 2.6e-13
The worst z is a block of the "zeros" case whose four hops are silent: what is left there is the high-pass's slow mode, a small
part of the state when the silence began, so its relative error is that of the state times their ratio, in any float64 ordering.
Everywhere else, the DC case included, both restatements are within 1.1e-13 (z) of the 80-bit run.  Any correct float64 ordering may
differ from another by about this much, so the bar is 8 times the worst of the four, under the ceiling of 1e-9 that the definition
sets as a condition: BAR = 4.16e-11 relative on energies, and (10 / ln 10) BAR = 1.8e-10 absolute on lufs.
tests/test_loudness_host.py re-measures and holds both restatements to MEASURED."""
import functools
import math

import numpy as np

LANES = 64
MEASURED = 5.2e-12          # the worst of the four figures above
BAR = 8 * MEASURED          # 4.16e-11
CEILING = 1e-9
assert BAR <= CEILING
LUFS_BAR = 10.0 / math.log(10.0) * BAR
GATE_MARGIN = 1e-6
ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)


# ---------------------------------------------------------------- the design formulas
def design(fs):
    """-> (b0, b1, b2, a1, a2, c1, c2): the shelf's numerator and denominator and the high-pass denominator (its numerator is 1, -2, 1)."""
    pi = 3.141592653589793
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(pi * f0 / fs)
    Vh = math.pow(10.0, G / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    b0, b1, b2 = (Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0
    a1, a2 = 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    c1, c2 = 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0
    return b0, b1, b2, a1, a2, c1, c2


def biquads(fs):
    """The same as scipy-style (b, a) pairs: [(shelf b, shelf a), (high-pass b, high-pass a)]."""
    b0, b1, b2, a1, a2, c1, c2 = design(fs)
    return [(np.array([b0, b1, b2]), np.array([1.0, a1, a2])), (np.array([1.0, -2.0, 1.0]), np.array([1.0, c1, c2]))]


def samples(x):
    """A recording as the library reads it, in float64: float32 as it lies, int16 PCM as (float)s / 32768."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return (x.astype(np.float32) / np.float32(32768)).astype(np.float64)
    assert x.dtype == np.float32, x.dtype
    return x.astype(np.float64)


def step(c, x, s):
    """One sample through the cascade (two transposed direct form II biquads), in the dtype of the operands; s = [z1, z2, w1, w2] is
    replaced; returns y."""
    b0, b1, b2, a1, a2, c1, c2 = c
    v = b0 * x + s[0]
    s[0] = (b1 * x - a1 * v) + s[1]
    s[1] = b2 * x - a2 * v
    y = v + s[2]
    s[2] = (-2.0 * v - c1 * y) + s[3]
    s[3] = v - c2 * y
    return y


# ---------------------------------------------------------------- the plain recurrence
def plain(xs, fs, dtype):
    """Hop energies of every recording of ``xs`` by the plain sample recurrence in ``dtype``; the recordings run side by side (shorter
    ones end early: their later hops are not taken).  -> list of (floor(L / H),) arrays of ``dtype``."""
    H = fs // 10
    nh = [len(x) // H for x in xs]
    R, N = len(xs), max(nh) * H
    X = np.zeros((N, R), dtype)
    for r, x in enumerate(xs):
        X[:nh[r] * H, r] = samples(x)[:nh[r] * H]
    c = tuple(dtype(v) for v in design(fs))
    s = [np.zeros(R, dtype) for _ in range(4)]
    E = np.zeros((max(nh), R), dtype)
    acc = np.zeros(R, dtype)
    for n in range(N):
        y = step(c, X[n], s)
        acc += y * y
        if (n + 1) % H == 0:
            E[n // H] = acc
            acc = np.zeros(R, dtype)
    return [E[:nh[r], r].copy() for r in range(R)]


def blocks(E, H):
    """z_j = (((E_j + E_{j+1}) + E_{j+2}) + E_{j+3}) / (4 H), j < len(E) - 3."""
    E = np.asarray(E)
    return (((E[:-3] + E[1:-2]) + E[2:-1]) + E[3:]) / E.dtype.type(4 * H)


def truth(xs, fs):
    """-> (hop energies, block energies z) per recording, np.longdouble."""
    E = plain(xs, fs, np.longdouble)
    return E, [blocks(e, fs // 10) for e in E]


def plain64(xs, fs):
    E = plain(xs, fs, np.float64)
    return E, [blocks(e, fs // 10) for e in E]


# ---------------------------------------------------------------- the device's formulation
def power(fs, n):
    """A^n (4, 4) float64: binary powering in np.longdouble, rounded once (csrc/loudness.h loud_power)."""
    b0, b1, b2, a1, a2, c1, c2 = (np.longdouble(v) for v in design(fs))
    one, zero, two = np.longdouble(1), np.longdouble(0), np.longdouble(2)
    base = [[-a1, one, zero, zero], [-a2, zero, zero, zero], [-two - c1, zero, -c1, one], [one - c2, zero, -c2, zero]]
    acc = [[one if i == j else zero for j in range(4)] for i in range(4)]

    def mul(x, y):
        out = [[zero] * 4 for _ in range(4)]
        for i in range(4):
            for j in range(4):
                s = zero
                for k in range(4):
                    s = s + x[i][k] * y[k][j]
                out[i][j] = s
        return out

    while n > 0:
        if n & 1:
            acc = mul(acc, base)
        base = mul(base, base)
        n >>= 1
    return np.array([[float(v) for v in row] for row in acc], np.float64)


def advance(M, e, s):
    """s <- M s + e, every row left to right; s, e: lists of four arrays (or floats)."""
    return [(((M[i][0] * s[0] + M[i][1] * s[1]) + M[i][2] * s[2]) + M[i][3] * s[3]) + e[i] for i in range(4)]


def device64(x, fs):
    """-> (hop energies, z) of ONE recording, float64, by the launches of csrc/k_loudness.hip."""
    H = fs // 10
    nh = len(x) // H
    p = -(-H // LANES)
    q = H % p
    c = design(fs)
    Ap, Aq, AH = power(fs, p).tolist(), power(fs, q).tolist(), power(fs, H).tolist()
    X = np.zeros((nh, LANES * p))
    X[:, :H] = samples(x)[:nh * H].reshape(nh, H)
    X = X.reshape(nh, LANES, p)
    valid = (np.arange(LANES)[:, None] * p + np.arange(p)[None, :]) < H  # (lane, i)
    # launch 1: every piece from zero state, then the lanes in order
    e = [np.zeros((nh, LANES)) for _ in range(4)]
    for i in range(p):
        t = [v.copy() for v in e]
        step(c, X[:, :, i], t)
        e = [np.where(valid[None, :, i], tv, ev) for tv, ev in zip(t, e)]

    def lane_scan(s):
        starts = [np.zeros((nh, LANES)) for _ in range(4)]
        for l in range(LANES):
            n = min(p, H - l * p)
            if n <= 0:
                break
            for k in range(4):
                starts[k][:, l] = s[k]
            s = advance(Ap if n == p else Aq, [v[:, l] for v in e], s)
        return starts, s

    _, hop_e = lane_scan([np.zeros(nh) for _ in range(4)])
    # launch 2: the hops in order
    hop_s = [np.zeros(nh) for _ in range(4)]
    s = [0.0, 0.0, 0.0, 0.0]
    for h in range(nh):
        for k in range(4):
            hop_s[k][h] = s[k]
        s = advance(AH, [float(hop_e[k][h]) for k in range(4)], s)
    # launch 3: true start states, second sweep, butterfly over the lanes
    st, _ = lane_scan(hop_s)
    acc = np.zeros((nh, LANES))
    for i in range(p):
        t = [v.copy() for v in st]
        y = step(c, X[:, :, i], t)
        m = valid[None, :, i]
        st = [np.where(m, tv, sv) for tv, sv in zip(t, st)]
        acc = np.where(m, acc + y * y, acc)
    o = LANES // 2
    while o > 0:
        acc = acc + acc[:, np.arange(LANES) ^ o]
        o >>= 1
    E = acc[:, 0].copy()
    return E, blocks(E, H)


# ---------------------------------------------------------------- gates
def gate(z):
    """Both gates in the z domain -> (lufs, kept), in the dtype of z; -inf and 0 when no block survives, NaN and 0 for a non-finite z."""
    z = np.asarray(z)
    if not np.isfinite(z).all():
        return float("nan"), 0
    a = z > z.dtype.type(ABS_GATE)
    if not a.any():
        return float("-inf"), 0
    rel = z.dtype.type(0.1) * (z[a].sum() / z.dtype.type(int(a.sum())))
    k = a & (z > rel)
    if not k.any():
        return float("-inf"), 0
    return float(z.dtype.type(-0.691) + z.dtype.type(10.0) * np.log10(z[k].sum() / z.dtype.type(int(k.sum())))), int(k.sum())


def gate_margin(z):
    """The smallest relative distance of a block of ``z`` from either threshold (inf if the relative gate is undefined)."""
    z = np.asarray(z, np.longdouble)
    m = float(np.abs(z / np.longdouble(ABS_GATE) - 1).min())
    a = z > np.longdouble(ABS_GATE)
    if a.any():
        rel = np.longdouble(0.1) * (z[a].sum() / np.longdouble(int(a.sum())))
        m = min(m, float(np.abs(z / rel - 1).min()))
    return m


def assert_gate_margin(z, name=""):
    m = gate_margin(z)
    assert m >= GATE_MARGIN, (name, m)


# ---------------------------------------------------------------- the GPU test inputs
def _pcm(x):
    return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """-> a tuple of (name, fs, recording): float32 or int16 arrays, seeded.  Per rate the recordings form one pool."""
    rng = np.random.RandomState(1770)
    out = []

    def noise(n, sigma=0.1):
        return (sigma * rng.randn(n)).astype(np.float32)

    for fs in (8000, 16000):
        H = fs // 10
        for k, L in enumerate((4 * H, 4 * H + 1, 5 * H - 1, 5 * H)):
            x = noise(L, 0.05 + 0.05 * k)
            out.append((f"len{L}", fs, _pcm(x) if k % 2 else x))
    H = 800
    for k, nh in enumerate((4, 5, 63, 64, 65, 255, 256, 257)):
        x = noise(nh * H + (37 * k) % H) * (1.0 + 0.5 * np.sin(np.arange(nh * H + (37 * k) % H) / 3000.0)).astype(np.float32)
        out.append((f"hops{nh}", 8000, _pcm(x) if k % 3 == 1 else x))
    fs, H = 16000, 1600
    x = noise(30 * H + 7)
    x[11 * H + 3:16 * H + 5] = 0.0                      # exact zeros: hops 12 .. 15 are silent, block 12 lies under the absolute gate
    out.append(("zeros", fs, x))
    x = noise(30 * H + 11)
    x[8 * H:20 * H] *= np.float32(0.01)                 # 40 dB under the rest: above -70 LUFS, under the relative gate
    out.append(("quiet40", fs, x))
    out.append(("under70", fs, noise(12 * H + 1, 1e-5)))  # wholly under the absolute gate: -inf
    x = noise(20 * H + 5, 0.02) + np.float32(0.2)       # a DC offset of ten deviations
    out.append(("dc", fs, x))
    out.append(("pcm_dc", fs, _pcm(noise(9 * H + 801, 0.02) + np.float32(0.05))))
    out.append(("r44100", 44100, noise(5 * 4410 + 100)))
    out.append(("r48000", 48000, _pcm(noise(6 * 4800 - 1))))
    return tuple(out)


def rates():
    return sorted({fs for _, fs, _ in gpu_cases()})


@functools.lru_cache(maxsize=None)
def truth_of_cases():
    """{name: (hop energies, z)} of every GPU input in np.longdouble, computed once per process, one sample loop per rate."""
    res = {}
    for fs in rates():
        named = [(n, x) for n, f, x in gpu_cases() if f == fs]
        E, Z = truth([x for _, x in named], fs)
        for (n, _), e, z in zip(named, E, Z):
            res[n] = (e, z)
    return res


def signal_hops(E, H):
    """The hops whose energies are compared one by one (see THE BAR): those whose mean square is above the absolute gate."""
    return np.asarray(E, np.float64) / H > ABS_GATE


def rel_dev(got, want):
    got, want = np.asarray(got, np.longdouble), np.asarray(want, np.longdouble)
    return float(np.max(np.abs(got - want) / np.abs(want))) if len(want) else 0.0


def measure():
    """-> {"plain64": (z, hops), "device64": (z, hops)}: the worst relative deviations from ``truth`` over ``gpu_cases()``."""
    tr = truth_of_cases()
    out = {"plain64": [0.0, 0.0], "device64": [0.0, 0.0]}
    for fs in rates():
        named = [(n, x) for n, f, x in gpu_cases() if f == fs]
        pe, pz = plain64([x for _, x in named], fs)
        for i, (n, x) in enumerate(named):
            de, dz = device64(x, fs)
            keep = signal_hops(tr[n][0], fs // 10)
            for key, e, z in (("plain64", pe[i], pz[i]), ("device64", de, dz)):
                out[key][0] = max(out[key][0], rel_dev(z, tr[n][1]))
                out[key][1] = max(out[key][1], rel_dev(e[keep], tr[n][0][keep]))
    return {k: tuple(v) for k, v in out.items()}
