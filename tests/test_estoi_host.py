"""Host side of extended STOI: the float64 oracle (tests/estoi_oracle.py) on the properties the definition has by construction, the
segment counts and the chunk-ownership rule the device stage is cut by, the four C entries' declarations, bindings and refusals, and the
tracker's seventh column through ``record`` alone.  None of it touches a device."""
import csv
import ctypes
import os
import re

import numpy as np
import pytest

from tests import estoi_oracle as E
from tests import metrics_oracle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = 11
SYMBOLS = {"rtfs_estoi_workspace_bytes": "size_t", "rtfs_estoi_f32": "int", "rtfs_estoi_many_workspace_bytes": "size_t",
           "rtfs_estoi_many_f32": "int"}


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


def _pair(L=32000, fs=16000, seed=0, noise=0.5, **kw):
    rng = np.random.default_rng(seed)
    x = M.speech_like(rng, L, fs, **kw)
    y = (x + noise * rng.standard_normal(L)).astype(np.float32)
    return x, y


# ---------------------------------------------------------------- the oracle
def test_identical_estimate_scores_one():
    x, _ = _pair(gaps=[(0.4, 0.7)])
    assert abs(E.estoi(x, x, 16000) - 1.0) < 1e-12


def test_zero_estimate_and_zero_clean_score_exactly_zero():
    x, y = _pair(seed=1)
    z = np.zeros_like(x)
    assert E.estoi(x, z, 16000) == 0.0
    assert E.estoi(z, y, 16000) == 0.0
    assert E.estoi(z, z, 16000) == 0.0


def test_scale_of_the_estimate_does_not_matter():
    x, y = _pair(seed=2)
    d = E.estoi(x, y, 16000)
    assert 0.1 < d < 0.99
    for c in (7.5, 1e-3):
        assert abs(E.estoi(x, c * y.astype(np.float64), 16000) - d) < 1e-12


def test_fewer_than_30_frames_gives_1e_5():
    x, y = _pair(L=6000, seed=3)  # 3750 samples at 10 kHz: 27 STFT frames
    assert E.estoi(x, y, 16000) == 1e-5
    assert E.estoi_from_bands(np.ones((15, 29)), np.ones((15, 29))) == 1e-5
    assert E.estoi_from_bands(np.ones((15, 30)), np.ones((15, 30))) == 0.0  # constant bands: every norm is zero, nothing is NaN


def test_estoi_falls_as_noise_is_added():
    x, _ = _pair(seed=4)
    n = np.random.default_rng(5).standard_normal(x.shape)
    ds = [E.estoi(x, x + a * n, 16000) for a in (0.05, 0.3, 1.0, 3.0)]
    assert all(a > b for a, b in zip(ds, ds[1:])), ds


@pytest.mark.parametrize("L,J", E.SEGMENT_LENGTHS)
def test_segment_counts(L, J):
    x, y = E.noise_pair(L, 500 + J)
    e = M.frame_energies(x.astype(np.float64))
    K0 = -(-(L - 256) // 128)
    kept, margin = M.kept_frames(x, 10000)
    # every frame is kept, far from the 40 dB threshold: a windowed frame of stationary noise has an energy spread of about +-0.5 dB
    # per standard deviation, so 5 dB between the loudest and the quietest frame is ten of them
    assert kept == K0 == len(e) and margin > 35.0 and e.max() - e.min() < 5.0
    assert E.n_segments(x, 10000) == J == max(0, K0 - 30)
    d = E.estoi(x, y, 10000)
    assert d == 1e-5 if J == 0 else 0.3 < d < 1.0


def _gpu_test_signals():
    """(clean, estimate, fs) of every oracle comparison in tests/test_hip_estoi.py."""
    from tests.test_hip_estoi import CASES
    from tests.test_hip_metrics import _case
    for B, L, fs, seed, extra in CASES.values():
        x, y = _case(B, L, fs, seed, **extra)
        for b in range(B):
            yield x[b], y[b], fs
    for L, J in E.SEGMENT_LENGTHS:
        yield E.noise_pair(L, 500 + J) + (10000,)


def test_pystoi_noise_terms_move_d_by_less_than_1e_12():
    worst, n = 0.0, 0
    for i, (x, y, fs) in enumerate(_gpu_test_signals()):
        x_tob, y_tob, _ = M.prepare(x, y, fs)  # the band values once; the noise enters after them
        d = E.estoi_from_bands(x_tob, y_tob)
        dn = E.estoi_from_bands(x_tob, y_tob, noise=np.random.default_rng(900 + i))
        worst, n = max(worst, abs(d - dn)), n + 1
    print(f"pystoi's two noise terms move d by at most {worst:.2e} over {n} signals")
    assert n == 54 and worst < 1e-12


def test_chunk_ownership_partitions_the_segments():
    for J in range(1, 2001):
        planned = E.planned_chunks(J)
        owners = [E.chunk_owner(s) for s in range(J)]
        assert owners == sorted(owners) and owners[-1] < planned          # every owner is a planned chunk
        counts = np.bincount(owners, minlength=planned)
        assert counts.sum() == J and counts.max() <= 18                    # a partition; slots 0 .. 17 suffice
        # the kernel's closed form of a chunk's range: [ceil(256 c / 15), min(J, ceil(256 (c + 1) / 15)))
        for c in range(planned):
            lo, hi = -(-256 * c // 15), min(J, -(-256 * (c + 1) // 15))
            assert max(0, hi - lo) == counts[c] and all(o == c for o in owners[lo:hi])
    assert E.planned_chunks(18) == 2 and E.chunk_owner(17) == 0           # the last planned chunk owns no segment
    assert E.planned_chunks(35) == 3 and E.chunk_owner(34) == 1


# ---------------------------------------------------------------- the C entries
def test_symbols_in_header_bindings_and_library():
    from rtfs_net_amd import _lib
    with open(os.path.join(ROOT, "include", "rtfs_amd.h")) as f:
        header = f.read()
    for name, res in SYMBOLS.items():
        decl = re.search(r"\b" + res + " " + name + r"\(([^;]*)\);", header)
        assert decl, name
        fn = getattr(lib(), name)  # exported and bound (an integer-only size query is wrapped in a memoising cache)
        assert name in _lib.SIGNATURES and getattr(fn, "__wrapped__", fn).argtypes == _lib.SIGNATURES[name][1]
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    from rtfs_net_amd import metrics
    import rtfs_net_amd
    assert rtfs_net_amd.estoi is metrics.estoi and rtfs_net_amd.estoi_many is metrics.estoi_many


def _plan(Ls, n_src=1, fs=16000):
    R = len(Ls)
    table = (ctypes.c_int * (COLS * (R + 1)))()
    nbytes = ctypes.c_size_t(0)
    assert lib().rtfs_score_many_plan((ctypes.c_longlong * R)(*Ls), R, n_src, fs, table, ctypes.byref(nbytes)) == 0
    return table, nbytes.value


def test_workspace_sizes():
    L_ = lib()
    for B, L, fs in ((1, 32000, 16000), (3, 32003, 16000), (2, 4000, 16000), (3, 20001, 10000)):
        base = L_.rtfs_stoi_workspace_bytes(B, L, fs)
        L10 = -(-5 * L // 8) if fs == 16000 else L
        J = -(-(L10 - 256) // 128) - 30
        nchunk = max(1, E.planned_chunks(J))
        assert L_.rtfs_estoi_workspace_bytes(B, L, fs, 0) == base                      # ESTOI alone: the classic workspace
        assert L_.rtfs_estoi_workspace_bytes(B, L, fs, 1) == -(-base // 256) * 256 + 8 * B * nchunk
    for fs in (8000, 44100, 0):
        assert L_.rtfs_estoi_workspace_bytes(2, 32000, fs, 0) == 0 and L_.rtfs_estoi_workspace_bytes(2, 32000, fs, 1) == 0
    assert L_.rtfs_estoi_workspace_bytes(1, 409, 16000, 1) == 0
    # pooled: the plan's own size alone; with classic one more region of 8 * (total of column 9) bytes at the next multiple of 256
    for Ls, n_src, fs in (([410, 6554, 1639], 1, 16000), ([6553, 410, 32769, 64003], 2, 16000), ([257, 4097, 6273, 20001], 1, 10000)):
        tab, nbytes = _plan(Ls, n_src, fs)
        R = len(Ls)
        cc_total = tab[9 * (R + 1) + R]
        assert L_.rtfs_estoi_many_workspace_bytes(tab, R, 0) == nbytes
        assert L_.rtfs_estoi_many_workspace_bytes(tab, R, 1) == -(-nbytes // 256) * 256 + 8 * cc_total
        assert L_.rtfs_estoi_many_workspace_bytes(tab, R + 1, 1) == 0 and L_.rtfs_estoi_many_workspace_bytes(None, R, 1) == 0


def test_refusals_come_before_any_device_is_touched():
    L_ = lib()
    ws = L_.rtfs_estoi_workspace_bytes(2, 32000, 16000, 1)
    n0 = L_.rtfs_debug_launch_count()
    for fs in (8000, 22050, 44100, 48000, 0, -16000):
        assert L_.rtfs_estoi_f32(8, 8, 2, 32000, fs, 8, ws, 8, 8, 8, None) == -4
    assert L_.rtfs_estoi_f32(None, 8, 2, 32000, 16000, 8, ws, 8, 8, 8, None) == -4
    assert L_.rtfs_estoi_f32(8, 8, 2, 32000, 16000, 8, ws, None, 8, 8, None) == -4
    assert L_.rtfs_estoi_f32(8, 8, 2, 32000, 16000, 8, ws, 8, None, None, None) == -4
    assert L_.rtfs_estoi_f32(8, 8, 2, 409, 16000, 8, ws, 8, 8, 8, None) == -1
    assert L_.rtfs_estoi_f32(8, 8, 0, 32000, 16000, 8, ws, 8, 8, 8, None) == -1
    assert L_.rtfs_estoi_f32(8, 8, 2, 32000, 16000, 8, 100, 8, None, 8, None) == -2
    # a workspace sized for ESTOI alone is too small once classic STOI is wanted as well
    assert L_.rtfs_estoi_f32(8, 8, 2, 32000, 16000, 8, L_.rtfs_estoi_workspace_bytes(2, 32000, 16000, 0), 8, 8, 8, None) == -2
    tab, nbytes = _plan([32000, 410])
    both = L_.rtfs_estoi_many_workspace_bytes(tab, 2, 1)
    assert both > nbytes
    assert L_.rtfs_estoi_many_f32(None, 8, 8, tab, 2, 1, 16000, 8, both, 8, 8, 8, None) == -4
    assert L_.rtfs_estoi_many_f32(8, 8, 8, None, 2, 1, 16000, 8, both, 8, 8, 8, None) == -4
    assert L_.rtfs_estoi_many_f32(8, 8, 8, tab, 2, 1, 16000, 8, both, None, 8, 8, None) == -4
    assert L_.rtfs_estoi_many_f32(8, 8, 8, tab, 2, 1, 10000, 8, both, 8, 8, 8, None) == -4   # a plan made for other arguments
    assert L_.rtfs_estoi_many_f32(8, 8, 8, tab, 2, 2, 16000, 8, both, 8, 8, 8, None) == -4
    assert L_.rtfs_estoi_many_f32(8, 8, 8, tab, 3, 1, 16000, 8, both, 8, 8, 8, None) == -4
    assert L_.rtfs_estoi_many_f32(8, 8, 8, tab, 2, 1, 16000, 8, nbytes - 1, 8, None, 8, None) == -2
    assert L_.rtfs_estoi_many_f32(8, 8, 8, tab, 2, 1, 16000, 8, both - 1, 8, 8, 8, None) == -2  # the tenth region is checked too
    assert L_.rtfs_debug_launch_count() == n0


def test_python_entries_refuse_like_stoi():
    import torch
    from rtfs_net_amd.metrics import estoi, estoi_many, stoi
    x = torch.zeros(1, 32000)
    with pytest.raises(ValueError, match="fs must be"):
        estoi(x, x, 8000)
    with pytest.raises(ValueError, match="same"):
        estoi(x, torch.zeros(1, 31999))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        estoi(x, x)
    with pytest.raises(ValueError, match="estoi"):
        stoi(x, x, 16000, extended=True)
    with pytest.raises(ValueError, match="fs must be"):
        estoi_many([x[0]], [x[0]], fs=8000)
    with pytest.raises(ValueError, match="recording 1 has 409 samples"):
        estoi_many([x[0], torch.zeros(409)], [x[0], torch.zeros(409)], with_classic=True)
    with pytest.raises(ValueError, match="no CPU fallback"):
        estoi_many([x[0]], [x[0]])


# ---------------------------------------------------------------- the tracker through record alone
def _vals(n, cols):
    rng = np.random.default_rng(6)
    v = np.stack([-rng.uniform(5, 15, n), rng.uniform(-12, -3, n), -rng.uniform(4, 14, n), rng.uniform(-11, -2, n),
                  rng.uniform(0.5, 0.95, n), rng.uniform(0.3, 0.9, n)], 1).astype(np.float32)
    return v[:, :cols], list(rng.uniform(1.5, 3.5, n))


def test_tracker_without_estoi_is_the_reference_format(tmp_path):
    from rtfs_net_amd.metrics import ALLMetricsTracker
    from tests.test_metrics_host import _RefTracker
    vals, pesqs = _vals(7, 5)
    keys = [f"utt{i}" for i in range(7)]
    ours, ref = tmp_path / "ours.csv", tmp_path / "ref.csv"
    t, r = ALLMetricsTracker(str(ours), estoi=False), _RefTracker(str(ref))
    assert not hasattr(t, "all_estois")
    t.record(keys[:3], vals[:3], pesqs[:3])
    t.record(keys[3:], vals[3:], pesqs[3:])
    for i in range(7):
        r(keys[i], *(float(v) for v in vals[i, :4]), pesqs[i], float(vals[i, 4]))
    for a, b in ((t.get_mean(), r.get_mean()), (t.get_std(), r.get_std())):
        assert list(a) == list(b)
        np.testing.assert_array_equal(np.array(list(a.values())), np.array(list(b.values())))
    with pytest.raises(ValueError, match="takes 5"):
        t.record(["x"], _vals(1, 6)[0], [1.0])
    t.final()
    r.final()
    assert ours.read_text() == ref.read_text()


def test_tracker_with_estoi_has_a_seventh_column(tmp_path):
    from rtfs_net_amd.metrics import ALLMetricsTracker
    vals, pesqs = _vals(7, 6)
    keys = [f"utt{i}" for i in range(7)]
    p5, p6 = tmp_path / "five.csv", tmp_path / "six.csv"
    t5, t6 = ALLMetricsTracker(str(p5)), ALLMetricsTracker(str(p6), estoi=True)
    t5.record(keys, vals[:, :5], pesqs)
    t6.record(keys[:4], vals[:4], pesqs[:4])
    t6.record(keys[4:], vals[4:], pesqs[4:])
    with pytest.raises(ValueError, match="takes 6"):
        t6.record(["x"], vals[:1, :5], [1.0])
    assert t6.all_estois == [float(v) for v in vals[:, 5]]
    mean, std = t6.get_mean(), t6.get_std()
    assert list(mean) == list(std) == ["sdr", "sdr_i", "si-snr", "si-snr_i", "pesq", "stoi", "estoi"]
    assert mean["estoi"] == np.mean([float(v) for v in vals[:, 5]]) and std["estoi"] == np.std([float(v) for v in vals[:, 5]])
    for k, v in t5.get_mean().items():
        assert mean[k] == v and std[k] == t5.get_std()[k]
    t5.final()
    t6.final()
    rows5, rows6 = list(csv.DictReader(open(p5))), list(csv.DictReader(open(p6)))
    assert list(rows6[0]) == ["snt_id", "sdr", "sdr_i", "si-snr", "si-snr_i", "pesq", "stoi", "estoi"]
    assert [r["snt_id"] for r in rows6] == keys + ["avg", "std"]
    for a, b in zip(rows5, rows6):  # the six reference columns are text-identical with and without the seventh
        assert all(b[k] == v for k, v in a.items())
    assert [float(r["estoi"]) for r in rows6[:7]] == [float(v) for v in vals[:, 5]]
    assert float(rows6[7]["estoi"]) == mean["estoi"] and float(rows6[8]["estoi"]) == std["estoi"]
