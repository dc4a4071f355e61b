"""Host side of BSS-eval SDR: the float64 oracle (tests/bss_oracle.py) -- the definition (LU solve, explicit convolution, time-domain
energies) against the cheap route the device takes (Levinson, closed-form energies) over every case set of the GPU tests, and the
properties the figure has by construction -- then the C entries' declarations, bindings, workspace sizes and refusals through ctypes,
and the tracker's two columns through ``record`` alone.  None of it touches a device.
Measured: max |sdr_lu - sdr_moments| = 1.8e-8 dB over the 111 pairs (bound 1e-6); condition numbers of Toeplitz(r) 2.0 .. 4.5e5."""
import csv
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from tests import bss_oracle as O
from tests import metrics_oracle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = 11
SYMBOLS = {"rtfs_bss_sdr_workspace_bytes": "size_t", "rtfs_bss_sdr_f32": "int", "rtfs_bss_sdr_many_workspace_bytes": "size_t",
           "rtfs_bss_sdr_many_f32": "int", "rtfs_debug_bss_f64": "int"}


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- the oracle
def test_definition_and_moment_route_agree_on_every_case():
    worst, n = 0.0, 0
    for name, s, e in O.all_pairs():
        a, b = O.sdr_lu(s, e), O.sdr_moments(s, e)
        n += 1
        if len(s) == 1:  # one sample: every estimate is a multiple of the reference, the fit is perfect
            assert a >= 120.0 and b >= 120.0, (name, a, b)
            continue
        assert np.isfinite(a) and np.isfinite(b) and a <= 61.0, (name, a, b)
        worst = max(worst, abs(a - b))
        assert abs(a - b) <= 1e-6, (name, a, b)
    print(f"max |sdr_lu - sdr_moments| = {worst:.2e} dB over {n} pairs")
    assert n == 111


@functools.lru_cache(maxsize=None)
def _speech(seed=0, L=32000):
    return M.speech_like(np.random.default_rng(seed), L, 16000)


def _noisy(s, seed, level=0.1):
    nz = np.random.default_rng(seed).standard_normal(len(s))
    return (s + level * np.linalg.norm(s) / np.linalg.norm(nz) * nz).astype(np.float32)


def test_scale_of_estimate_and_reference_does_not_matter():
    s = _speech(1, 8000)
    e = _noisy(s, 2)
    want = O.sdr_lu(s, e)
    assert 15.0 < want < 25.0
    for c in (1e-3, 1e3):
        for fn in (O.sdr_lu, O.sdr_moments):
            assert abs(fn(s, (c * e.astype(np.float64))) - want) <= 1e-6
            assert abs(fn((c * s.astype(np.float64)), e) - want) <= 1e-6


def test_a_delay_of_100_samples_is_allowed_and_one_of_600_is_not():
    s = _speech(3)
    for delay, lo, hi in ((100, 20.0, np.inf), (600, -np.inf, 0.0)):
        e = np.concatenate([np.zeros(delay, np.float32), s[:-delay]])
        for fn in (O.sdr_lu, O.sdr_moments):
            v = fn(s, e)
            assert lo < v < hi, (delay, v)
        assert O.snr(s, e) < 0.0, (delay, O.snr(s, e))  # plain SNR, the tracker's "sdr" column, is ruined either way


def test_a_causal_64_tap_fir_of_the_reference_scores_above_40_db():
    s = _speech(4)
    h = np.random.default_rng(5).standard_normal(64) * np.exp(-np.arange(64) / 12.0)
    e = np.convolve(s.astype(np.float64), h)[:len(s)].astype(np.float32)
    assert O.sdr_lu(s, e) > 40.0 and O.sdr_moments(s, e) > 40.0
    assert O.snr(s, e) < 10.0


def test_silent_and_perfect_rows():
    s = _speech(6, 4097)
    z = np.zeros_like(s)
    assert O.sdr_moments(z, s) == -np.inf and np.isnan(O.sdr_moments(z, z)) and np.isnan(O.sdr_moments(s, z))
    v = O.sdr_moments(s, s)
    assert v == np.inf or v >= 120.0


def test_permutation_rule():
    assert O.best_perm([[9.0, 1.0], [2.0, 8.0]]) == [0, 1]
    assert O.best_perm([[1.0, 9.0], [8.0, 2.0]]) == [1, 0]
    assert O.best_perm([[5.0, 5.0], [5.0, 5.0]]) == [0, 1]                       # a tie: the first in itertools order
    assert O.best_perm([[0, 9, 0], [0, 0, 9], [9, 0, 0]]) == [2, 0, 1]           # perm[j] = the estimate assigned to clean j
    assert O.best_perm([[np.nan, 1.0], [2.0, 3.0]]) == [0, 1]                    # a NaN mean never replaces, never is replaced
    for n in (2, 3, 4):
        clean, est, mix, shuffle = O.source_case(n)
        want = [shuffle.index(j) for j in range(n)]
        sdr, sdr_i, perm = O.bss_eval(clean, est, mix, fn=O.sdr_moments)
        assert perm == want and (sdr > 10.0).all() and (sdr_i > 10.0).all(), (n, perm, want, sdr, sdr_i)
        clean, est, mix, shuffle = O.source_case(n, True)
        perm_i = O.bss_eval(clean, est, None, fn=O.sdr_moments)[2]
        assert perm_i.index(0) < perm_i.index(1)                                 # identical estimates 0 and 1: the first maximum


# ---------------------------------------------------------------- the C entries
def test_symbols_in_header_bindings_and_library():
    from rtfs_net_amd import _lib
    with open(os.path.join(ROOT, "include", "rtfs_amd.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name, res in SYMBOLS.items():
        decl = re.search(r"\b" + res + " " + name + r"\(([^;]*)\);", header)
        assert decl, name
        fn = getattr(lib(), name)
        assert name in _lib.SIGNATURES and getattr(fn, "__wrapped__", fn).argtypes == _lib.SIGNATURES[name][1]
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    import rtfs_net_amd
    from rtfs_net_amd import metrics
    assert rtfs_net_amd.bss_sdr is metrics.bss_sdr and rtfs_net_amd.bss_sdr_many is metrics.bss_sdr_many


def _plan(Ls, n_src=1, fs=16000):
    R = len(Ls)
    table = (ctypes.c_int * (COLS * (R + 1)))()
    nbytes = ctypes.c_size_t(0)
    assert lib().rtfs_score_many_plan((ctypes.c_longlong * R)(*Ls), R, n_src, fs, table, ctypes.byref(nbytes)) == 0
    return table, nbytes.value


def _bytes(G, rows, n, with_mix):
    """three regions, each starting at a multiple of 256: partials (G, n, 1 + NR, 512), sums of squares (G, NR), num / den (rows, n, NR, 2)"""
    NR, up = n + with_mix, lambda v: -(-v // 256) * 256
    return up(up(8 * G * n * (1 + NR) * 512) + 8 * G * NR) + 8 * rows * n * NR * 2


def test_workspace_sizes():
    L_ = lib()
    for B, n, L, wm in ((1, 1, 1, 0), (1, 1, 4096, 1), (3, 2, 4097, 1), (5, 4, 32003, 0), (256, 1, 32000, 1)):
        assert L_.rtfs_bss_sdr_workspace_bytes(B, n, L, wm) == _bytes(B * -(-L // O.CHUNK), B, n, wm), (B, n, L, wm)
    for bad in ((0, 1, 100, 0), (1, 0, 100, 0), (1, 5, 100, 1), (1, 1, 0, 0)):
        assert L_.rtfs_bss_sdr_workspace_bytes(*bad) == 0
    for Ls, n in (([410, 6554, 1639], 1), ([6553, 410, 32769, 64003], 2), ([4096, 4097, 8193], 4)):
        tab, nbytes = _plan(Ls, n)
        R = len(Ls)
        G = sum(-(-L // O.CHUNK) for L in Ls)
        assert tab[10 * (R + 1) + R] == G
        for wm in (0, 1):
            assert L_.rtfs_bss_sdr_many_workspace_bytes(tab, R, wm) == _bytes(G, R, n, wm)
        assert L_.rtfs_bss_sdr_many_workspace_bytes(tab, R + 1, 1) == 0 and L_.rtfs_bss_sdr_many_workspace_bytes(None, R, 1) == 0
        _, again = _plan(Ls, n)
        assert again == nbytes  # the plan's own workspace is what it was


def test_refusals_come_before_any_device_is_touched():
    L_ = lib()
    ws = L_.rtfs_bss_sdr_workspace_bytes(2, 2, 5000, 1)
    n0 = L_.rtfs_debug_launch_count()
    ok = dict(clean=8, est=8, mix=8, B=2, n=2, L=5000, ws=8, nb=ws, sdr=8, sdr_i=8, perm=8)

    def block(**kw):
        a = {**ok, **kw}
        return L_.rtfs_bss_sdr_f32(a["clean"], a["est"], a["mix"], a["B"], a["n"], a["L"], a["ws"], a["nb"], a["sdr"], a["sdr_i"], a["perm"], None)

    for key in ("clean", "est", "ws", "sdr", "sdr_i", "perm"):
        assert block(**{key: None}) == -4, key
    for kw in (dict(B=0), dict(B=-1), dict(L=0), dict(n=0), dict(n=5)):
        assert block(**kw) == -4, kw
    assert block(nb=ws - 1) == -2 and block(nb=0) == -2
    assert block(mix=None, sdr_i=None, nb=L_.rtfs_bss_sdr_workspace_bytes(2, 2, 5000, 0) - 1) == -2
    # the debug entry: the same refusals, and its own pointers and solver form
    dbg = lambda form=0, r=8, nb=ws: L_.rtfs_debug_bss_f64(8, 8, 8, 2, 2, 5000, 8, nb, 8, 8, 8, form, r, 8, 8, 8, None)  # noqa: E731
    assert dbg(r=None) == -4 and dbg(form=128) == -4 and dbg(form=-1) == -4 and dbg(nb=ws - 1) == -2
    tab, _ = _plan([32000, 410], 2)
    own = L_.rtfs_bss_sdr_many_workspace_bytes(tab, 2, 1)

    def many(mixes=8, cleans=8, ests=8, table=8, plan=tab, R=2, n=2, fs=16000, ws_=8, nb=own, sdr=8, sdr_i=8, perm=8):
        return L_.rtfs_bss_sdr_many_f32(mixes, cleans, ests, table, plan, R, n, fs, ws_, nb, sdr, sdr_i, perm, None)

    for kw in (dict(cleans=None), dict(ests=None), dict(table=None), dict(plan=None), dict(ws_=None), dict(sdr=None), dict(sdr_i=None),
               dict(perm=None), dict(fs=10000), dict(fs=8000), dict(n=1), dict(n=5), dict(R=3), dict(R=0)):
        assert many(**kw) == -4, kw
    assert many(nb=own - 1) == -2
    assert many(mixes=None, sdr_i=None, nb=L_.rtfs_bss_sdr_many_workspace_bytes(tab, 2, 0) - 1) == -2
    assert L_.rtfs_debug_launch_count() == n0


def test_python_entries_refuse_before_any_launch():
    import torch
    from rtfs_net_amd.metrics import bss_sdr, bss_sdr_many
    x = torch.zeros(2, 2, 1000)
    with pytest.raises(ValueError, match="same"):
        bss_sdr(x, torch.zeros(2, 2, 999))
    with pytest.raises(ValueError, match="same"):
        bss_sdr(x, x[0])
    with pytest.raises(ValueError, match="mix must be"):
        bss_sdr(x, x, torch.zeros(2, 999))
    with pytest.raises(ValueError, match="mix must be"):
        bss_sdr(x[0, 0], x[0, 0], torch.zeros(1, 1000))
    with pytest.raises(ValueError, match="n_src must be 1 .. 4"):
        bss_sdr(torch.zeros(1, 5, 100), torch.zeros(1, 5, 100))
    with pytest.raises(ValueError, match="float32"):
        bss_sdr(x.double(), x.double())
    with pytest.raises(ValueError, match="float32"):
        bss_sdr(x, x, torch.zeros(2, 1000, dtype=torch.float64))
    with pytest.raises(ValueError, match="empty"):
        bss_sdr(torch.zeros(2, 2, 0), torch.zeros(2, 2, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bss_sdr(x, x)
    with pytest.raises(ValueError, match=r"recording 1 has 409 samples.*410 \.\. 2\^26"):
        bss_sdr_many([x[0], torch.zeros(2, 409)], [x[0], torch.zeros(2, 409)])
    with pytest.raises(ValueError, match="recording 1 has 5 clean"):
        bss_sdr_many([x[0], torch.zeros(5, 1000)], [x[0], torch.zeros(5, 1000)])
    with pytest.raises(ValueError, match="equally long"):
        bss_sdr_many([x[0]], [x[0]], [torch.zeros(999)])
    with pytest.raises(ValueError, match="float32"):
        bss_sdr_many([x[0].double()], [x[0].double()])
    with pytest.raises(ValueError, match="no CPU fallback"):
        bss_sdr_many([x[0]], [x[0]])


# ---------------------------------------------------------------- the tracker through record alone
def _vals(n, cols):
    rng = np.random.default_rng(6)
    v = np.stack([-rng.uniform(5, 15, n), rng.uniform(-12, -3, n), -rng.uniform(4, 14, n), rng.uniform(-11, -2, n),
                  rng.uniform(0.5, 0.95, n), rng.uniform(0.3, 0.9, n), rng.uniform(8, 30, n), rng.uniform(3, 20, n)], 1).astype(np.float32)
    return v[:, cols], list(rng.uniform(1.5, 3.5, n))


def test_tracker_without_the_option_writes_what_it_wrote(tmp_path):
    from rtfs_net_amd.metrics import ALLMetricsTracker
    from tests.test_metrics_host import _RefTracker
    vals, pesqs = _vals(7, [0, 1, 2, 3, 4])
    keys = [f"utt{i}" for i in range(7)]
    ours, ref = tmp_path / "ours.csv", tmp_path / "ref.csv"
    t, r = ALLMetricsTracker(str(ours), bss_sdr=False), _RefTracker(str(ref))
    assert not hasattr(t, "all_bss_sdrs") and not hasattr(t, "all_bss_sdrs_i")
    t.record(keys, vals, pesqs)
    for i in range(7):
        r(keys[i], *(float(v) for v in vals[i, :4]), pesqs[i], float(vals[i, 4]))
    with pytest.raises(ValueError, match="takes 5"):
        t.record(["x"], _vals(1, [0, 1, 2, 3, 4, 6, 7])[0], [1.0])
    t.final()
    r.final()
    assert ours.read_bytes() == ref.read_bytes()


@pytest.mark.parametrize("estoi", [False, True])
def test_tracker_columns(tmp_path, estoi):
    from rtfs_net_amd.metrics import ALLMetricsTracker
    base_cols = [0, 1, 2, 3, 4] + ([5] if estoi else [])
    vals, pesqs = _vals(7, base_cols + [6, 7])
    keys = [f"utt{i}" for i in range(7)]
    pa, pb = tmp_path / "without.csv", tmp_path / "with.csv"
    ta, tb = ALLMetricsTracker(str(pa), estoi=estoi), ALLMetricsTracker(str(pb), estoi=estoi, bss_sdr=True)
    ta.record(keys, vals[:, :len(base_cols)], pesqs)
    tb.record(keys[:4], vals[:4], pesqs[:4])
    tb.record(keys[4:], vals[4:], pesqs[4:])
    with pytest.raises(ValueError, match=f"takes {len(base_cols) + 2}"):
        tb.record(["x"], vals[:1, :len(base_cols)], [1.0])
    with pytest.raises(ValueError, match=f"takes {len(base_cols) + 2}"):
        tb.record(["x"], np.concatenate([vals[:1], vals[:1, :1]], 1), [1.0])
    want, want_i = [float(v) for v in vals[:, -2]], [float(v) for v in vals[:, -1]]
    assert tb.all_bss_sdrs == want and tb.all_bss_sdrs_i == want_i and min(want) > 0  # positive dB, as they came
    if estoi:
        assert tb.all_estois == [float(v) for v in vals[:, 5]]
    names = ["sdr", "sdr_i", "si-snr", "si-snr_i", "pesq", "stoi"] + (["estoi"] if estoi else []) + ["bss_sdr", "bss_sdr_i"]
    mean, std = tb.get_mean(), tb.get_std()
    assert list(mean) == list(std) == names
    assert mean["bss_sdr"] == np.mean(want) and std["bss_sdr"] == np.std(want)
    assert mean["bss_sdr_i"] == np.mean(want_i) and std["bss_sdr_i"] == np.std(want_i)
    for k, v in ta.get_mean().items():
        assert mean[k] == v and std[k] == ta.get_std()[k]
    ta.final()
    tb.final()
    rows_a, rows_b = list(csv.DictReader(open(pa))), list(csv.DictReader(open(pb)))
    assert list(rows_b[0]) == ["snt_id"] + names
    assert [r["snt_id"] for r in rows_b] == keys + ["avg", "std"]
    for a, b in zip(rows_a, rows_b):  # the other columns, avg and std rows included, are text-identical with and without the two
        assert all(b[k] == v for k, v in a.items())
    assert [float(r["bss_sdr"]) for r in rows_b[:7]] == want and [float(r["bss_sdr_i"]) for r in rows_b[:7]] == want_i
    assert float(rows_b[7]["bss_sdr"]) == mean["bss_sdr"] and float(rows_b[8]["bss_sdr"]) == std["bss_sdr"]
    assert float(rows_b[7]["bss_sdr_i"]) == mean["bss_sdr_i"] and float(rows_b[8]["bss_sdr_i"]) == std["bss_sdr_i"]
