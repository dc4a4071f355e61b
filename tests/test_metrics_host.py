"""CPU tests of the evaluation metrics: the float64 STOI oracle (tests/metrics_oracle.py, a restatement of pystoi 0.4.1) on the
properties pystoi has by construction, and ALLMetricsTracker's CSV logic against a literal transcription of the reference's
src/metrics/allwrapper.py."""
import csv

import numpy as np
import pytest
import scipy.signal

from tests import metrics_oracle as M


def _pair(L=32000, fs=16000, seed=0, **kw):
    rng = np.random.default_rng(seed)
    x = M.speech_like(rng, L, fs, **kw)
    return x, rng


def test_identical_signals_give_one():
    x, _ = _pair(gaps=[(0.4, 0.7)])
    assert abs(M.stoi(x, x, 16000) - 1.0) < 1e-12


def test_scale_of_the_estimate_does_not_matter():
    x, rng = _pair(seed=1)
    y = (x + 0.5 * rng.standard_normal(x.shape)).astype(np.float32)
    d = M.stoi(x, y, 16000)
    for c in (1e-3, 0.37, 25.0):
        assert abs(M.stoi(x, (c * y.astype(np.float64)), 16000) - d) < 1e-12


def test_stoi_falls_as_noise_is_added():
    x, rng = _pair(seed=2)
    n = rng.standard_normal(x.shape)
    ds = [M.stoi(x, x + a * n, 16000) for a in (0.05, 0.3, 1.0, 3.0)]
    assert all(a > b for a, b in zip(ds, ds[1:])), ds
    assert ds[0] > 0.9 and ds[-1] < 0.6


def test_short_input_returns_1e_5():
    x, rng = _pair(L=6000, seed=3)  # 3750 samples at 10 kHz: 28 frames, 27 STFT frames < 30
    assert M.stoi(x, x + 0.1 * rng.standard_normal(x.shape), 16000) == 1e-5


def test_zero_estimate_and_all_zero_clean():
    x, rng = _pair(seed=4)
    assert M.stoi(x, np.zeros_like(x), 16000) == 0.0
    z = np.zeros_like(x)
    assert M.kept_frames(z, 16000)[0] == len(M.frame_energies(M.resample_oct(z.astype(np.float64), 10000, 16000)))  # every frame kept
    assert M.stoi(z, x, 16000) == 0.0


def test_resample_filter_and_alignment():
    h = M.resample_window_oct(5, 8)
    assert len(h) == 581
    w = h / h.sum()
    assert abs(w.sum() - 1.0) < 1e-14
    rng = np.random.default_rng(5)
    for L in (32000, 32003, 131200):
        x = rng.standard_normal(L)
        y = M.resample_oct(x, 10000, 16000)
        assert len(y) == -(-L * 5 // 8)
        np.testing.assert_array_equal(y, scipy.signal.resample_poly(x, 5, 8, window=w))
        # the direct form the kernel evaluates: output n = sum_j 5 w[290 + 8n - 5j] x[j] over the input in range
        for n in (0, 1, 57, len(y) // 2, len(y) - 2, len(y) - 1):
            j = np.arange(max(0, -(-(8 * n - 290) // 5)), min(L - 1, (8 * n + 290) // 5) + 1)
            assert abs(np.sum(5 * w[290 + 8 * n - 5 * j] * x[j]) - y[n]) < 1e-12


def test_band_matrix_edges():
    obm, cf = M.thirdoct(10000, 512, 15, 150)
    assert obm.shape == (15, 257)
    f = np.linspace(0, 10000, 513)[:257]
    for i, (lo, hi) in enumerate(M.band_edges()):
        k = float(i)
        assert lo == np.argmin((f - 150 * 2 ** ((2 * k - 1) / 6)) ** 2)
        assert hi == np.argmin((f - 150 * 2 ** ((2 * k + 1) / 6)) ** 2)
        assert obm[i].sum() == hi - lo
    assert M.band_edges()[0][0] == 7 and M.band_edges()[-1][1] == 219  # the bins csrc/k_stoi.hip computes


def test_frame_ranges_exclude_the_last_full_frame():
    x = np.arange(256 + 128 * 3, dtype=np.float64)  # starts 0, 128, 256 (384 = len - 256 excluded)
    assert M.frames(x).shape == (3, 256)
    xs, ys, mask = M.remove_silent_frames(x, x)
    assert len(xs) == (mask.sum() - 1) * 128 + 256


# ---------------------------------------------------------------- ALLMetricsTracker CSV logic
class _RefTracker:
    """allwrapper.py:19-134 transcribed, with the metric calls replaced by given per-row values (the loss-sign tensors' .item())."""

    def __init__(self, save_file):
        self.all_sdrs, self.all_sdrs_i, self.all_sisnrs, self.all_sisnrs_i, self.all_pesqs, self.all_stois = [], [], [], [], [], []
        csv_columns = ["snt_id", "sdr", "sdr_i", "si-snr", "si-snr_i", "pesq", "stoi"]
        self.results_csv = open(save_file, "w")
        self.writer = csv.DictWriter(self.results_csv, fieldnames=csv_columns)
        self.writer.writeheader()

    def __call__(self, key, sdr, sdr_i, sisnr, sisnr_i, _pesq, _stoi):
        row = {"snt_id": key, "sdr": sdr, "sdr_i": sdr_i, "si-snr": -sisnr, "si-snr_i": -sisnr_i, "pesq": _pesq, "stoi": _stoi}
        self.writer.writerow(row)
        self.all_sdrs.append(-sdr)
        self.all_sdrs_i.append(-sdr_i)
        self.all_sisnrs.append(-sisnr)
        self.all_sisnrs_i.append(-sisnr_i)
        self.all_pesqs.append(_pesq)
        self.all_stois.append(_stoi)

    def get_mean(self):
        return {"sdr": np.mean(self.all_sdrs), "sdr_i": np.mean(self.all_sdrs_i), "si-snr": np.mean(self.all_sisnrs),
                "si-snr_i": np.mean(self.all_sisnrs_i), "pesq": np.mean(self.all_pesqs), "stoi": np.mean(self.all_stois)}

    def get_std(self):
        return {"sdr": np.std(self.all_sdrs), "sdr_i": np.std(self.all_sdrs_i), "si-snr": np.std(self.all_sisnrs),
                "si-snr_i": np.std(self.all_sisnrs_i), "pesq": np.std(self.all_pesqs), "stoi": np.std(self.all_stois)}

    def final(self):
        for name, red in (("avg", np.mean), ("std", np.std)):
            self.writer.writerow({"snt_id": name, "sdr": red(np.array(self.all_sdrs)), "sdr_i": red(np.array(self.all_sdrs_i)),
                                  "si-snr": red(np.array(self.all_sisnrs)), "si-snr_i": red(np.array(self.all_sisnrs_i)),
                                  "pesq": red(np.array(self.all_pesqs)), "stoi": red(np.array(self.all_stois))})
        self.results_csv.close()


@pytest.mark.parametrize("with_pesq", [True, False])
def test_tracker_csv_matches_reference_transcription(tmp_path, with_pesq):
    from rtfs_net_amd.metrics import ALLMetricsTracker
    rng = np.random.default_rng(6)
    vals = np.stack([-rng.uniform(5, 15, 7), rng.uniform(-12, -3, 7), -rng.uniform(4, 14, 7), rng.uniform(-11, -2, 7),
                     rng.uniform(0.5, 0.95, 7)], 1).astype(np.float32)
    pesqs = list(rng.uniform(1.5, 3.5, 7)) if with_pesq else [float("nan")] * 7
    keys = [f"utt{i}" for i in range(7)]
    ours, ref = tmp_path / "ours.csv", tmp_path / "ref.csv"
    t = ALLMetricsTracker(str(ours))
    r = _RefTracker(str(ref))
    t.record(keys[:3], vals[:3], pesqs[:3])  # two batches: rows accumulate across update calls
    t.record(keys[3:], vals[3:], pesqs[3:])
    for i in range(7):
        r(keys[i], *(float(v) for v in vals[i, :4]), pesqs[i], float(vals[i, 4]))
    for a, b in ((t.get_mean(), r.get_mean()), (t.get_std(), r.get_std())):
        assert list(a) == list(b)
        np.testing.assert_array_equal(np.array(list(a.values())), np.array(list(b.values())))
    t.final()
    r.final()
    assert ours.read_text() == ref.read_text()
    rows = list(csv.DictReader(open(ours)))
    assert [x["snt_id"] for x in rows] == keys + ["avg", "std"]
    assert float(rows[0]["sdr"]) < 0 and float(rows[0]["si-snr"]) > 0  # the reference's mixed signs
    assert float(rows[-2]["sdr"]) > 0 and float(rows[-2]["si-snr"]) > 0
    assert (rows[-2]["pesq"] == "nan") != with_pesq


def test_stoi_refuses_extended_and_other_rates():
    import torch
    from rtfs_net_amd.metrics import stoi
    x = torch.zeros(1, 32000)
    with pytest.raises(ValueError):
        stoi(x, x, 16000, extended=True)
    with pytest.raises(ValueError):
        stoi(x, x, 8000)
