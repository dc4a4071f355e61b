"""rtfs_stoi_f32 (csrc/k_stoi.hip) and rtfs_net_amd.metrics (stoi, ALLMetricsTracker) on the MI355X against the float64 oracle
(tests/metrics_oracle.py, a restatement of pystoi 0.4.1; parity with pystoi itself is unpinned).

Inputs are speech-like (amplitude-modulated noise with gaps at -60 dB and at exact zero) so that silence removal really removes frames;
each case asserts that no clean frame lies within 1e-3 dB of the 40 dB threshold, so the kept-frame count is decided the same way in
float32 and float64 and must match exactly.  The poisoned runs (every workspace and output starting as NaN or 3.4e38 bytes, guard bands
after each workspace) are made here because tests/test_hip_poisoned.py lists its own files."""
import csv

import numpy as np
import pytest
import torch

from tests import metrics_oracle as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4
MARGIN_DB = 1e-3


def _case(B, L, fs, seed, heavy_gap_rows=(), zero_est_rows=(), zero_clean_rows=()):
    """(clean, est) float32 (B, L): per row a speech-like clean signal with a -60 dB gap and an exact-zero gap, the estimate = clean +
    noise of a per-row level.  heavy_gap_rows are silent for about 70 % of their length."""
    rng = np.random.default_rng(seed)
    dur = L / fs
    xs, ys = [], []
    for b in range(B):
        if b in heavy_gap_rows:
            gaps, zgaps = [(0.05 * dur, 0.45 * dur)], [(0.5 * dur, 0.8 * dur)]
        else:
            gaps, zgaps = [(0.30 * dur, 0.42 * dur)], [(0.6 * dur, 0.68 * dur)]
        x = M.speech_like(rng, L, fs, gaps=gaps, zero_gaps=zgaps, level=rng.uniform(0.05, 2.0))
        y = (x + rng.uniform(0.02, 1.5) * np.std(x) * rng.standard_normal(L)).astype(np.float32)
        if b in zero_est_rows:
            y[:] = 0
        if b in zero_clean_rows:
            x[:] = 0
        xs.append(x)
        ys.append(y)
    return np.stack(xs), np.stack(ys)


def _oracle(x, y, fs):
    d, kept = [], []
    for b in range(x.shape[0]):
        k, margin = M.kept_frames(x[b], fs)
        if x[b].any():
            assert margin >= MARGIN_DB, f"row {b}: a frame lies {margin:.2e} dB from the silence threshold; redraw the case"
        d.append(M.stoi(x[b], y[b], fs))
        kept.append(k)
    return np.array(d), np.array(kept)


def _run(x, y, fs):
    from rtfs_net_amd.metrics import stoi
    d, kept = stoi(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), fs, return_kept=True)
    torch.cuda.synchronize()
    return d.cpu().numpy().astype(np.float64), kept.cpu().numpy()


CASES = {  # name: (B, L, fs, seed, extra)
    "b1_2s": (1, 32000, 16000, 10, {}),
    "b3_2s_odd": (3, 32003, 16000, 11, {"heavy_gap_rows": (1,)}),
    "b3_short_1e5": (3, 4000, 16000, 12, {}),  # 2500 samples at 10 kHz: at most 17 STFT frames
    "b2_odd_len": (2, 17005, 16000, 13, {"heavy_gap_rows": (0,)}),
    "b1_8s": (1, 131200, 16000, 14, {}),
    "b3_10k": (3, 20001, 10000, 15, {"heavy_gap_rows": (2,)}),
    "b2_10k_short": (2, 3000, 10000, 16, {}),
    "b32_2s": (32, 32000, 16000, 17, {"heavy_gap_rows": (5, 20)}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_stoi_matches_oracle(name):
    B, L, fs, seed, extra = CASES[name]
    x, y = _case(B, L, fs, seed, **extra)
    d_ref, k_ref = _oracle(x, y, fs)
    d, k = _run(x, y, fs)
    np.testing.assert_array_equal(k, k_ref)
    err = np.abs(d - d_ref).max()
    print(f"{name}: max |d - oracle| = {err:.3e}, kept {k.tolist()[:4]} of {len(M.frames(np.zeros(-(-L * 5 // 8) if fs == 16000 else L)))}")
    assert err <= TOL, (d, d_ref)
    if "heavy_gap_rows" in extra:  # more than half of the frames removed
        K0 = len(M.frames(np.zeros(-(-L * 5 // 8) if fs == 16000 else L)))
        assert all(k[r] < K0 / 2 for r in extra["heavy_gap_rows"])
    if "short" in name:
        assert (d == np.float32(1e-5)).all()


def test_rows_do_not_depend_on_the_batch():
    x, y = _case(5, 32000, 16000, 20, heavy_gap_rows=(3,))
    d, k = _run(x, y, 16000)
    for b in range(5):
        d1, k1 = _run(x[b:b + 1], y[b:b + 1], 16000)
        assert d1[0] == d[b] and k1[0] == k[b]


def test_scaled_zero_and_silent_rows():
    x, y = _case(4, 32000, 16000, 21, zero_est_rows=(1,), zero_clean_rows=(2,))
    d_ref, k_ref = _oracle(x, y, 16000)
    d, k = _run(x, y, 16000)
    np.testing.assert_array_equal(k, k_ref)
    assert d[1] == 0.0 and d_ref[1] == 0.0  # zero estimate: 0, not NaN
    assert d[2] == 0.0 and d_ref[2] == 0.0  # all-zero clean: every frame kept, finite energies
    assert k[2] == len(M.frames(np.zeros(20000)))
    assert np.abs(d - d_ref).max() <= TOL
    for c in (1e-3, 7.5):
        dc, kc = _run(x, (c * y).astype(np.float32), 16000)
        np.testing.assert_array_equal(kc, k)
        assert np.abs(dc - d).max() <= 1e-5, (c, dc, d)


def test_one_dimensional_input():
    from rtfs_net_amd.metrics import stoi
    x, y = _case(1, 32000, 16000, 22)
    d = stoi(torch.from_numpy(x[0]).to(DEV), torch.from_numpy(y[0]).to(DEV))
    assert d.shape == () and abs(float(d) - M.stoi(x[0], y[0], 16000)) <= TOL


def test_other_rates_refused_before_any_launch():
    import ctypes
    from rtfs_net_amd import _lib
    lib = _lib.load()
    x = torch.zeros(2, 32000, device=DEV)
    d = torch.zeros(2, device=DEV)
    k = torch.zeros(2, device=DEV, dtype=torch.int32)
    ws = torch.zeros(lib.rtfs_stoi_workspace_bytes(2, 32000, 16000), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    for fs in (8000, 22050, 44100, 48000, 0, -16000):
        n0 = lib.rtfs_debug_launch_count()
        rc = lib.rtfs_stoi_f32(_lib.ptr(x), _lib.ptr(x), 2, 32000, fs, _lib.ptr(ws), ws.numel(), _lib.ptr(d), _lib.ptr(k),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == -4 and lib.rtfs_debug_launch_count() == n0
        assert lib.rtfs_stoi_workspace_bytes(2, 32000, fs) == 0
    assert lib.rtfs_stoi_f32(_lib.ptr(x), _lib.ptr(x), 2, 409, 16000, _lib.ptr(ws), ws.numel(), _lib.ptr(d), _lib.ptr(k), None) == -1
    assert lib.rtfs_stoi_f32(_lib.ptr(x), _lib.ptr(x), 2, 32000, 16000, _lib.ptr(ws), 100, _lib.ptr(d), _lib.ptr(k), None) == -2


def test_graph_capture_replays_eager():
    from rtfs_net_amd.metrics import stoi
    x, y = _case(4, 32000, 16000, 23, heavy_gap_rows=(2,))
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    eager, keager = stoi(xd, yd, return_kept=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        stoi(xd, yd)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, kout = stoi(xd, yd, return_kept=True)
    xd.copy_(torch.from_numpy(x[::-1].copy()))  # new inputs in the captured buffers
    yd.copy_(torch.from_numpy(y[::-1].copy()))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager.flip(0)) and torch.equal(kout, keager.flip(0))


@pytest.mark.parametrize("byte", [0xFF, 0x7F], ids=["nan", "big"])
def test_poisoned_workspace_and_outputs(monkeypatch, byte):
    from rtfs_net_amd import _lib
    runs = [(_case(3, 32003, 16000, 30, heavy_gap_rows=(1,), zero_est_rows=(2,)), 16000), (_case(2, 4000, 16000, 31), 16000),
            (_case(3, 20001, 10000, 32, zero_clean_rows=(0,)), 10000)]
    clean = [_run(x, y, fs) for (x, y), fs in runs]
    monkeypatch.setattr(_lib, "_POISON", byte)
    for ((x, y), fs), (d0, k0) in zip(runs, clean):
        d, k = _run(x, y, fs)  # _lib.check() verifies the guard band after the workspace
        np.testing.assert_array_equal(d, d0)
        np.testing.assert_array_equal(k, k0)
    x, y = runs[0][0]
    _tracker_rows(x, y, 16000, None)  # the tracker's launches under poison too (its own comparison is the test below)


def _tracker_rows(clean, est, fs, path):
    import tempfile
    from rtfs_net_amd.metrics import ALLMetricsTracker
    rng = np.random.default_rng(40)
    mix = (clean + 0.8 * rng.standard_normal(clean.shape) * clean.std()).astype(np.float32)
    with tempfile.TemporaryDirectory() as td:
        p = path or f"{td}/m.csv"
        t = ALLMetricsTracker(p)
        B = clean.shape[0]
        t.update_batch(torch.from_numpy(mix).to(DEV), torch.from_numpy(clean[:, None]).to(DEV), torch.from_numpy(est[:, None]).to(DEV),
                       [f"k{b}" for b in range(B)])
        mean, std = t.get_mean(), t.get_std()
        t.final()
        rows = list(csv.DictReader(open(p)))
    return mix, rows, mean, std


def test_tracker_update_batch_matches_oracle_composition():
    x, y = _case(8, 32000, 16000, 41, heavy_gap_rows=(4,))
    mix, rows, mean, std = _tracker_rows(x, y, 16000, None)
    assert [r["snt_id"] for r in rows] == [f"k{b}" for b in range(8)] + ["avg", "std"]
    acc = {k: [] for k in ("sdr", "sdr_i", "si-snr", "si-snr_i", "stoi")}
    for b in range(8):
        sisnr, sisnr_i, sdr, sdr_i, st = M.tracker_values(mix[b], x[b:b + 1], y[b:b + 1])
        want = {"sdr": sdr, "sdr_i": sdr_i, "si-snr": -sisnr, "si-snr_i": -sisnr_i, "stoi": st}
        for k, v in want.items():
            assert abs(float(rows[b][k]) - v) <= TOL * max(1.0, abs(v)), (b, k, rows[b][k], v)
        assert rows[b]["pesq"] == "nan"
        for k, v in (("sdr", -sdr), ("sdr_i", -sdr_i), ("si-snr", -sisnr), ("si-snr_i", -sisnr_i), ("stoi", st)):
            acc[k].append(v)
    for k, v in acc.items():
        assert abs(mean[k] - np.mean(v)) <= TOL * max(1.0, abs(np.mean(v))), k
        assert abs(std[k] - np.std(v)) <= TOL * max(1.0, abs(np.std(v))), k
        assert abs(float(rows[8][k]) - np.mean(v)) <= TOL * max(1.0, abs(np.mean(v))), k
    # __call__ is update_batch with B = 1, and a host pesq_fn receives (estimate, clean, 16000)
    import tempfile
    from rtfs_net_amd.metrics import ALLMetricsTracker
    seen = []
    with tempfile.TemporaryDirectory() as td:
        t = ALLMetricsTracker(f"{td}/one.csv", pesq_fn=lambda e, c, fs: seen.append((e, c, fs)) or 2.5)
        t(torch.from_numpy(mix[0]).to(DEV), torch.from_numpy(x[0:1]).to(DEV), torch.from_numpy(y[0:1]).to(DEV), "only")
        t.final()
        one = list(csv.DictReader(open(f"{td}/one.csv")))
    assert one[0]["snt_id"] == "only" and float(one[0]["pesq"]) == 2.5
    np.testing.assert_array_equal(seen[0][0], y[0])
    np.testing.assert_array_equal(seen[0][1], x[0])
    assert seen[0][2] == 16000
    for k in ("sdr", "sdr_i", "si-snr", "si-snr_i", "stoi"):
        assert abs(float(one[0][k]) - float(rows[0][k])) <= 1e-6 * max(1.0, abs(float(rows[0][k]))), k
