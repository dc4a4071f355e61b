"""Scoring recordings of different lengths in one pooled pass on the MI355X: rtfs_stoi_many_f32 / rtfs_sdr_many_f32 (csrc/k_stoi.hip,
csrc/k_score.hip) through metrics.stoi_many, metrics.sdr_many, ALLMetricsTracker.update_many and System.evaluate_many, against the
single-length entries (bit-equal STOI) and the float64 oracles (tests/metrics_oracle.py, a restatement of pystoi 0.4.1 whose parity with
pystoi itself is unpinned; oracle/loss_oracle.py).

Lengths sit where a stage's geometry changes (16 kHz): 410 (L10 = 257, one frame), 1638 / 1639 (L10 = 1024 / 1025: one resample
workgroup exactly, and one past), 6553 / 6554 (K0 = 30 / 31: with every frame kept the last length on the 1e-5 path and the first with
one 30-frame segment), 32769 (L10 = 20481), 32000 and 64003.  The 6553 / 6554 rows have no gaps and the oracle confirms that all K0
frames are kept; the others carry the -60 dB and exact-zero gaps of test_hip_metrics._case; 64003 is a heavy-gap row and 32000 has an
all-zero estimate.  Every case asserts on the oracle alone that no clean frame lies within 1e-3 dB of the silence threshold.  Tensors
are separate allocations; every third one is carved 1 or 3 floats past a 128-byte line of a larger buffer."""
import csv
import functools

import numpy as np
import pytest
import torch

from oracle.loss_oracle import pairwise_neg_sdr, pit_from_pw_mtx
from tests import metrics_oracle as M
from tests.test_hip_metrics import MARGIN_DB, TOL, _case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L16 = (410, 1638, 1639, 6553, 6554, 32769, 32000, 64003)
L10K = (257, 4096, 4097, 20001)
NO_GAPS = {(6553, 16000): 30, (6554, 16000): 31, (4096, 10000): 30, (4097, 10000): 31}  # (L, fs) -> K0, all kept
HEAVY, ZERO_EST = 64003, 32000
SEED = {16000: 100, 10000: 200}  # case r of a rate draws from SEED[fs] + r; chosen on the CPU so that every margin holds


def _n_frames(L, fs):
    L10 = -(-L * 5 // 8) if fs == 16000 else L
    return -(-(L10 - 256) // 128)


@functools.lru_cache(maxsize=None)
def pool(fs):
    """-> per recording (mix (L), clean (1, L), est (1, L)) float32 and the oracle's (d, kept); computed once, never changed."""
    recs, ref = [], []
    for r, L in enumerate(L16 if fs == 16000 else L10K):
        seed = SEED[fs] + r
        if (L, fs) in NO_GAPS:
            rng = np.random.default_rng(seed)
            x = M.speech_like(rng, L, fs, level=rng.uniform(0.05, 2.0))
            y = (x + rng.uniform(0.02, 1.5) * np.std(x) * rng.standard_normal(L)).astype(np.float32)
        else:
            xs, ys = _case(1, L, fs, seed, heavy_gap_rows=(0,) if L == HEAVY else (), zero_est_rows=(0,) if L == ZERO_EST else ())
            x, y = xs[0], ys[0]
        kept, margin = M.kept_frames(x, fs)
        assert margin >= MARGIN_DB, f"L = {L} at {fs}: a frame lies {margin:.2e} dB from the silence threshold; redraw the case"
        if (L, fs) in NO_GAPS:
            assert kept == NO_GAPS[(L, fs)] == _n_frames(L, fs), (L, kept)
        if L == HEAVY:
            assert kept < _n_frames(L, fs) / 2
        rng = np.random.default_rng(seed + 1000)
        mix = (x + 0.8 * np.std(x) * rng.standard_normal(L)).astype(np.float32)
        recs.append((mix, x[None].copy(), y[None].copy()))
        ref.append((M.stoi(x, y, fs), kept))
    return recs, ref


def carve(a, k):
    """a on the device as its own allocation; every third one starts 1 or 3 floats past a 128-byte line of a larger buffer."""
    a = np.ascontiguousarray(a)
    if k % 3 == 0:
        return torch.from_numpy(a).to(DEV)
    off = 32 + (1 if k % 3 == 1 else 3)
    buf = torch.zeros(a.size + 96, device=DEV)
    assert buf.data_ptr() % 128 == 0
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 128 == 4 * (off - 32)
    return t


def on_device(recs):
    return ([carve(m, 3 * r + 1) for r, (m, c, e) in enumerate(recs)], [carve(c, 3 * r + 2) for r, (m, c, e) in enumerate(recs)],
            [carve(e, 3 * r) for r, (m, c, e) in enumerate(recs)])


def host(*ts):
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in ts]
    return out[0] if len(out) == 1 else out


def close(got, want):
    return abs(float(got) - float(want)) <= TOL * max(1.0, abs(float(want)))


# ---------------------------------------------------------------- 1. stoi_many against stoi and the oracle
@pytest.mark.parametrize("fs", [16000, 10000])
def test_stoi_many_is_stoi_per_row_and_matches_the_oracle(fs):
    from rtfs_net_amd.metrics import stoi, stoi_many
    recs, ref = pool(fs)
    _, cleans, ests = on_device(recs)
    d, kept = host(*stoi_many(cleans, ests, fs, return_kept=True))
    assert d.shape == (len(recs),) and d.dtype == np.float32 and kept.dtype == np.int32
    for r, (c, e) in enumerate(zip(cleans, ests)):
        d1, k1 = host(*stoi(c[0], e[0], fs, return_kept=True))
        print(f"fs {fs} L {c.shape[1]}: d {d[r]!r} alone {d1!r} oracle {ref[r][0]!r} kept {kept[r]} / {ref[r][1]}")
        assert d[r].tobytes() == d1.tobytes() and kept[r] == k1, (r, d[r], d1)
        assert abs(float(d[r]) - ref[r][0]) <= TOL * max(1.0, abs(float(d[r]))), (r, d[r], ref[r][0])
        assert kept[r] == ref[r][1]
    lens = [c.shape[1] for c in cleans]
    short = [r for r, L in enumerate(lens) if _n_frames(L, fs) - 1 < 30]
    assert short and all(d[r] == np.float32(1e-5) for r in short)
    # rows may also come as (L): the same values
    d2 = host(stoi_many([c[0] for c in cleans], [e[0] for e in ests], fs))
    assert d2.tobytes() == d.tobytes()


# ---------------------------------------------------------------- 2. sdr_many against the tracker oracle
def test_sdr_many_matches_the_tracker_oracle():
    from rtfs_net_amd.metrics import sdr_many
    recs, _ = pool(16000)
    out, perm = host(*sdr_many(*on_device(recs)))
    assert out.shape == (len(recs), 4) and out.dtype == np.float32 and perm.shape == (len(recs), 1) and not perm.any()
    for r, (m, c, e) in enumerate(recs):
        sisnr, sisnr_i, sdr, sdr_i, _ = M.tracker_values(m, c, e)
        print(f"L {m.shape[0]}: got {out[r]} want {[sdr, sdr_i, sisnr, sisnr_i]}")
        for got, want in zip(out[r], (sdr, sdr_i, sisnr, sisnr_i)):
            assert close(got, want), (r, out[r], (sdr, sdr_i, sisnr, sisnr_i))


@functools.lru_cache(maxsize=None)
def pool2():
    """Three two-source mixtures: sources in order, sources swapped (best permutation (1, 0)), and swapped with estimate = clean + 1e-4
    noise (about 80 dB: the cancellation in |noise|^2)."""
    rng = np.random.default_rng(300)
    recs = []
    for L, swap, noise in ((4097, False, 0.3), (32003, True, 0.3), (12289, True, 1e-4)):
        c = np.stack([M.speech_like(rng, L, 16000, level=1.0), M.speech_like(rng, L, 16000, level=0.6)])
        e = (c + noise * c.std() * rng.standard_normal(c.shape)).astype(np.float32)
        e = np.ascontiguousarray(e[::-1]) if swap else e
        recs.append(((c[0] + c[1]).astype(np.float32), c, e))
    return recs


def test_sdr_many_two_sources_permutation_and_high_sdr():
    from rtfs_net_amd.metrics import sdr_many
    recs = pool2()
    out, perm = host(*sdr_many(*on_device(recs)))
    assert perm.shape == (3, 2)
    for r, (m, c, e) in enumerate(recs):
        want_perm = pit_from_pw_mtx(pairwise_neg_sdr(e[None], c[None], "sisdr"))[2][0]
        sisnr, sisnr_i, sdr, sdr_i, _ = M.tracker_values(m, c, e)
        print(f"L {m.shape[0]}: got {out[r]} perm {perm[r]} want {[sdr, sdr_i, sisnr, sisnr_i]} perm {want_perm}")
        np.testing.assert_array_equal(perm[r], want_perm)
        for got, want in zip(out[r], (sdr, sdr_i, sisnr, sisnr_i)):
            assert close(got, want), (r, out[r], (sdr, sdr_i, sisnr, sisnr_i))
    assert perm[0].tolist() == [0, 1] and perm[1].tolist() == [1, 0] and perm[2].tolist() == [1, 0]
    assert out[2, 2] < -70  # the high-SDR recording, loss sign


# ---------------------------------------------------------------- 3. pooling changes nothing
def _five(mixes, cleans, ests):
    from rtfs_net_amd.metrics import sdr_many, stoi_many
    out, d = host(sdr_many(mixes, cleans, ests)[0], stoi_many([c[0] for c in cleans], [e[0] for e in ests]))
    return np.concatenate([out, d[:, None]], 1)


def test_pooling_changes_nothing():
    mixes, cleans, ests = on_device(pool(16000)[0])
    pooled = _five(mixes, cleans, ests)
    rev = _five(mixes[::-1], cleans[::-1], ests[::-1])
    assert rev[::-1].tobytes() == pooled.tobytes()
    for r in range(len(mixes)):
        alone = _five(mixes[r:r + 1], cleans[r:r + 1], ests[r:r + 1])
        assert alone.tobytes() == pooled[r:r + 1].tobytes(), (r, alone, pooled[r])
    m2, c2, e2 = on_device(pool2())
    out = host(_sdr(m2, c2, e2))
    assert host(_sdr(m2[::-1], c2[::-1], e2[::-1]))[::-1].tobytes() == out.tobytes()
    for r in range(3):
        assert host(_sdr(m2[r:r + 1], c2[r:r + 1], e2[r:r + 1])).tobytes() == out[r:r + 1].tobytes()


def _sdr(m, c, e):
    from rtfs_net_amd.metrics import sdr_many
    return sdr_many(m, c, e)[0]


# ---------------------------------------------------------------- 4. update_many against __call__
def _tracker(tmp_path, name, feed, pesq_fn=None):
    from rtfs_net_amd.metrics import ALLMetricsTracker
    t = ALLMetricsTracker(str(tmp_path / name), pesq_fn=pesq_fn)
    feed(t)
    mean, std = t.get_mean(), t.get_std()
    t.final()
    return list(csv.DictReader(open(tmp_path / name))), mean, std


def test_update_many_leaves_the_tracker_as_calls_do(tmp_path):
    recs, _ = pool(16000)
    mixes, cleans, ests = on_device(recs)
    keys = [f"utt{r}" for r in range(len(recs))]
    seen = []

    def pesq(e, c, fs):
        seen.append((e, c, fs))
        return 1.0 + len(seen)

    many = _tracker(tmp_path, "many.csv", lambda t: t.update_many(mixes, cleans, ests, keys), pesq)
    n_many = len(seen)
    one = _tracker(tmp_path, "one.csv", lambda t: [t(m, c, e, k) for m, c, e, k in zip(mixes, cleans, ests, keys)], pesq)
    assert n_many == len(recs) == len(seen) - n_many
    for r, (m, c, e) in enumerate(recs):
        np.testing.assert_array_equal(seen[r][0], e[0])
        np.testing.assert_array_equal(seen[r][1], c[0])
        assert seen[r][2] == 16000
    rows, rows1 = many[0], one[0]
    assert [x["snt_id"] for x in rows] == [x["snt_id"] for x in rows1] == keys + ["avg", "std"]
    for a, b in zip(rows[:-2], rows1[:-2]):
        assert a["stoi"] == b["stoi"]  # text-identical
        assert float(a["pesq"]) == float(b["pesq"]) - len(recs)
    for a, b in zip(rows, rows1):
        for k in ("sdr", "sdr_i", "si-snr", "si-snr_i"):
            assert close(a[k], b[k]), (a["snt_id"], k, a[k], b[k])
    for got, want in ((many[1], one[1]), (many[2], one[2])):
        for k in ("sdr", "sdr_i", "si-snr", "si-snr_i", "stoi"):
            assert close(got[k], want[k]), (k, got[k], want[k])
    assert rows[-2]["stoi"] == rows1[-2]["stoi"] and rows[-1]["stoi"] == rows1[-1]["stoi"]


# ---------------------------------------------------------------- 5. poisoned workspace and outputs
@pytest.mark.parametrize("byte", [0xFF, 0x7F], ids=["nan", "big"])
def test_poisoned_workspace_and_outputs(monkeypatch, tmp_path, byte):
    from rtfs_net_amd import _lib
    from rtfs_net_amd.metrics import stoi_many
    mixes, cleans, ests = on_device(pool(16000)[0])
    m2, c2, e2 = on_device(pool2())
    _, c10, e10 = on_device(pool(10000)[0])

    def run():
        return (_five(mixes, cleans, ests), host(_sdr(m2, c2, e2)), host(*stoi_many(c10, e10, 10000, return_kept=True)))

    clean = run()
    monkeypatch.setattr(_lib, "_POISON", byte)
    poisoned = run()  # _lib.check() verifies the guard band after the workspace of every call
    for a, b in zip(clean, poisoned):
        for x, y in zip(a, b) if isinstance(a, list) else [(a, b)]:
            assert x.tobytes() == y.tobytes()
    rows = _tracker(tmp_path, "p.csv", lambda t: t.update_many(mixes, cleans, ests, list(range(len(mixes)))))[0]
    assert [float(r["stoi"]) for r in rows[:-2]] == [float(v) for v in clean[0][:, 4]]


# ---------------------------------------------------------------- 6. System.evaluate_many
def test_system_evaluate_many_is_separate_many_then_update_many(tmp_path):
    import rtfs_net_amd as R
    from oracle.params import make_inputs
    from tests.test_hip_longform import model
    system = R.System(audio_model=model(4)).eval()
    rng = np.random.default_rng(400)
    wavs, embs, cleans = [], [], []
    for r, L in enumerate((8000, 20480, 33000)):
        Tv = -(-L // 640)
        wav, emb = make_inputs(1, L, Tv, 410 + r)
        wavs.append(carve(wav[0], r))
        embs.append(torch.from_numpy(np.ascontiguousarray(emb[0])).to(DEV))
        cleans.append(carve(M.speech_like(rng, L, 16000)[None], r + 1))
    keys = ["a", "b", "c"]
    kw = dict(window=16000, hop=6400)  # the hop is a whole number of video frames (640 samples); 1, 2 and 4 windows
    want = system.separate_many(wavs, embs, **kw)
    got = []
    rows = _tracker(tmp_path, "eval.csv", lambda t: got.extend(system.evaluate_many(wavs, cleans, embs, keys, t, **kw)))
    assert len(got) == 3
    for g, w, wav in zip(got, want, wavs):
        assert tuple(g.shape) == (1, wav.shape[0]) and host(g).tobytes() == host(w).tobytes() and np.isfinite(host(g)).all()
    rows2 = _tracker(tmp_path, "upd.csv", lambda t: t.update_many(wavs, cleans, want, keys))
    assert rows[0] == rows2[0] and [r["snt_id"] for r in rows[0]] == keys + ["avg", "std"]
    for k in rows[1]:
        assert rows[1][k] == rows2[1][k] or (np.isnan(rows[1][k]) and np.isnan(rows2[1][k]))
