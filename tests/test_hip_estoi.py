"""Extended STOI on the MI355X: rtfs_estoi_f32 / rtfs_estoi_many_f32 (csrc/k_stoi.hip) through metrics.estoi, metrics.estoi_many and
ALLMetricsTracker(estoi=True), against the float64 oracle (tests/estoi_oracle.py: the published definition without pystoi's noise terms
and with the inverse of a zero norm taken as 0; agreement with the pystoi package itself is not measured, it is not installed) and
against the classic entries (bit-equal classic output from the combined call).

Signals: test_hip_metrics._case at that file's shapes (speech-like, gaps at -60 dB and at exact zero), and stationary Gaussian noise at
10 kHz at the nine lengths where the segment count crosses an edge of the work cut (estoi_oracle.SEGMENT_LENGTHS: J = 0, 1, 17, 18, 19,
35, 36, 256, 257; at J = 18 and 35 the last planned chunk owns no segment).  Kept-frame counts must be equal under MARGIN_DB.
Measured on the MI355X: max |estoi - oracle| 3.0e-8 over the seven cases and 2.9e-8 over the nine lengths, against TOL = 1e-4."""
import csv
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import estoi_oracle as E
from tests import metrics_oracle as M
from tests.test_hip_metrics import CASES as CLASSIC_CASES
from tests.test_hip_metrics import MARGIN_DB, TOL, _case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = {k: v for k, v in CLASSIC_CASES.items() if k != "b2_10k_short"}  # name: (B, L, fs, seed, extra)


def _oracle(x, y, fs):
    d, kept = [], []
    for b in range(x.shape[0]):
        k, margin = M.kept_frames(x[b], fs)
        if x[b].any():
            assert margin >= MARGIN_DB, f"row {b}: a frame lies {margin:.2e} dB from the silence threshold; redraw the case"
        d.append(E.estoi(x[b], y[b], fs))
        kept.append(k)
    return np.array(d), np.array(kept)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(*ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _run(x, y, fs, with_classic=False):
    """-> (estoi, kept) or (estoi, stoi, kept) as numpy (float32 kept as it is)"""
    from rtfs_net_amd.metrics import estoi
    return _host(*estoi(_dev(x), _dev(y), fs, return_kept=True, with_classic=with_classic))


def _stoi(x, y, fs):
    from rtfs_net_amd.metrics import stoi
    return _host(*stoi(_dev(x), _dev(y), fs, return_kept=True))


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("name", list(CASES))
def test_estoi_matches_oracle(name):
    B, L, fs, seed, extra = CASES[name]
    x, y = _case(B, L, fs, seed, **extra)
    d_ref, k_ref = _oracle(x, y, fs)
    d, dc, k = _run(x, y, fs, with_classic=True)
    assert d.dtype == np.float32 and d.shape == (B,)
    np.testing.assert_array_equal(k, k_ref)
    err = np.abs(d.astype(np.float64) - d_ref).max()
    print(f"{name}: max |estoi - oracle| = {err:.3e}, estoi {d[:3].tolist()}, kept {k.tolist()[:4]}")
    assert err <= TOL, (d, d_ref)
    d1, k1 = _run(x, y, fs)                      # alone: the same bits as from the combined call
    assert d1.tobytes() == d.tobytes() and (k1 == k).all()
    dc0, k0 = _stoi(x, y, fs)                    # the combined call's classic output is rtfs_stoi_f32's
    assert dc.tobytes() == dc0.tobytes() and (k0 == k).all()
    if "short" in name:
        assert (d == np.float32(1e-5)).all() and (dc == np.float32(1e-5)).all()


@functools.lru_cache(maxsize=None)
def segment_pool():
    """Per SEGMENT_LENGTHS entry (clean, estimate) at 10 kHz and the oracle's (d, kept); computed once, never changed."""
    recs, ref = [], []
    for L, J in E.SEGMENT_LENGTHS:
        x, y = E.noise_pair(L, 500 + J)
        kept, margin = M.kept_frames(x, 10000)
        assert margin >= MARGIN_DB and kept == J + 30 == -(-(L - 256) // 128), (L, kept)  # every frame kept
        recs.append((x, y))
        ref.append((E.estoi(x, y, 10000), kept))
    return recs, ref


def test_segment_count_edges_block_and_pooled():
    from rtfs_net_amd.metrics import estoi_many
    recs, ref = segment_pool()
    cleans, ests = [_dev(x) for x, _ in recs], [_dev(y) for _, y in recs]
    d, dc, kept = _host(*estoi_many(cleans, ests, 10000, return_kept=True, with_classic=True))
    d_alone = _host(estoi_many(cleans, ests, 10000))[0]
    assert d_alone.tobytes() == d.tobytes()
    worst = 0.0
    for r, ((x, y), (d_ref, k_ref)) in enumerate(zip(recs, ref)):
        d1, dc1, k1 = _run(x[None], y[None], 10000, with_classic=True)  # its own block call
        assert d1[0].tobytes() == d[r].tobytes() and dc1[0].tobytes() == dc[r].tobytes() and k1[0] == kept[r] == k_ref
        err = abs(float(d[r]) - d_ref)
        worst = max(worst, err)
        print(f"L {len(x)} J {E.SEGMENT_LENGTHS[r][1]}: estoi {d[r]!r} oracle {d_ref!r} |diff| {err:.3e} kept {kept[r]}")
        assert err <= TOL
        assert abs(float(dc[r]) - M.stoi(x, y, 10000)) <= TOL
    print(f"segment edges: max |estoi - oracle| = {worst:.3e}")
    assert d[0] == np.float32(1e-5) and all(v != np.float32(1e-5) for v in d[1:])


# ---------------------------------------------------------------- 2. bit equality
def test_pooled_rows_are_block_rows_and_classic_is_stoi():
    from rtfs_net_amd.metrics import estoi, estoi_many, stoi, stoi_many
    from tests.test_hip_score_many import on_device, pool
    for fs in (16000, 10000):
        _, cleans, ests = on_device(pool(fs)[0])
        d, dc, kept = _host(*estoi_many(cleans, ests, fs, return_kept=True, with_classic=True))
        ds, ks = _host(*stoi_many(cleans, ests, fs, return_kept=True))
        assert dc.tobytes() == ds.tobytes() and (kept == ks).all()
        assert _host(estoi_many(cleans, ests, fs))[0].tobytes() == d.tobytes()
        rev = _host(estoi_many(cleans[::-1], ests[::-1], fs))[0]
        assert rev[::-1].tobytes() == d.tobytes()            # the pool's order changes nothing
        for r, (c, e) in enumerate(zip(cleans, ests)):
            d1, dc1, k1 = _host(*estoi(c[0], e[0], fs, return_kept=True, with_classic=True))
            assert d1.shape == () and d1.tobytes() == d[r].tobytes() and k1 == kept[r], (fs, r, d1, d[r])
            assert dc1.tobytes() == _host(stoi(c[0], e[0], fs))[0].tobytes() == dc[r].tobytes()
            ref = E.estoi(c[0].cpu().numpy(), e[0].cpu().numpy(), fs)
            assert abs(float(d[r]) - ref) <= TOL, (fs, r, d[r], ref)


def test_rows_do_not_depend_on_the_batch():
    x, y = _case(5, 32000, 16000, 20, heavy_gap_rows=(3,))
    d, k = _run(x, y, 16000)
    for b in range(5):
        d1, k1 = _run(x[b:b + 1], y[b:b + 1], 16000)
        assert d1[0].tobytes() == d[b].tobytes() and k1[0] == k[b]


def test_scaled_zero_and_silent_rows():
    x, y = _case(4, 32000, 16000, 21, zero_est_rows=(1,), zero_clean_rows=(2,))
    d_ref, k_ref = _oracle(x, y, 16000)
    d, k = _run(x, y, 16000)
    np.testing.assert_array_equal(k, k_ref)
    assert d[1] == 0.0 and d_ref[1] == 0.0  # zero estimate: exactly 0, not NaN
    assert d[2] == 0.0 and d_ref[2] == 0.0  # all-zero clean: every frame kept, every norm zero
    assert np.abs(d - d_ref).max() <= TOL
    for c in (1e-3, 7.5):
        dc, kc = _run(x, (c * y).astype(np.float32), 16000)
        np.testing.assert_array_equal(kc, k)
        assert np.abs(dc.astype(np.float64) - d).max() <= 1e-5, (c, dc, d)


def test_one_dimensional_input():
    from rtfs_net_amd.metrics import estoi
    x, y = _case(1, 32000, 16000, 22)
    d = estoi(_dev(x[0]), _dev(y[0]))
    assert d.shape == () and abs(float(d) - E.estoi(x[0], y[0], 16000)) <= TOL


# ---------------------------------------------------------------- 3. refusals, graph capture
def test_refusals_come_before_any_launch():
    from rtfs_net_amd import _lib
    lib = _lib.load()
    x = torch.zeros(2, 32000, device=DEV)
    d, dc = torch.zeros(2, device=DEV), torch.zeros(2, device=DEV)
    k = torch.zeros(2, device=DEV, dtype=torch.int32)
    ws = torch.zeros(lib.rtfs_estoi_workspace_bytes(2, 32000, 16000, 1), dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n0 = lib.rtfs_debug_launch_count()
    P = _lib.ptr
    for fs in (8000, 22050, 44100, 48000, 0, -16000):
        assert lib.rtfs_estoi_f32(P(x), P(x), 2, 32000, fs, P(ws), ws.numel(), P(d), P(dc), P(k), st) == -4
        assert lib.rtfs_estoi_workspace_bytes(2, 32000, fs, 1) == 0
    assert lib.rtfs_estoi_f32(P(x), P(x), 2, 409, 16000, P(ws), ws.numel(), P(d), P(dc), P(k), st) == -1
    assert lib.rtfs_estoi_f32(P(x), P(x), 2, 32000, 16000, P(ws), 100, P(d), None, P(k), st) == -2
    alone = lib.rtfs_estoi_workspace_bytes(2, 32000, 16000, 0)
    assert lib.rtfs_estoi_f32(P(x), P(x), 2, 32000, 16000, P(ws), alone, P(d), P(dc), P(k), st) == -2
    assert lib.rtfs_estoi_f32(P(x), P(x), 2, 32000, 16000, P(ws), ws.numel(), None, P(dc), P(k), st) == -4
    # pooled: a plan made for other arguments, and a workspace without the tenth region
    plan = (ctypes.c_int * 33)()
    nbytes = ctypes.c_size_t(0)
    assert lib.rtfs_score_many_plan((ctypes.c_longlong * 2)(32000, 32000), 2, 1, 16000, plan, ctypes.byref(nbytes)) == 0
    both = lib.rtfs_estoi_many_workspace_bytes(plan, 2, 1)
    rows = torch.tensor([x[0].data_ptr(), x[1].data_ptr()], dtype=torch.int64, device=DEV)
    tab = torch.tensor(list(plan), dtype=torch.int32, device=DEV)
    wsm = torch.zeros(both, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    n0 = lib.rtfs_debug_launch_count()
    args = lambda fs, n, nb, dcp: (P(rows), P(rows), P(tab), plan, 2, n, fs, P(wsm), nb, P(d), dcp, P(k), st)  # noqa: E731
    assert lib.rtfs_estoi_many_f32(*args(10000, 1, both, P(dc))) == -4
    assert lib.rtfs_estoi_many_f32(*args(16000, 2, both, P(dc))) == -4
    assert lib.rtfs_estoi_many_f32(*args(16000, 1, nbytes.value, P(dc))) == -2
    assert lib.rtfs_estoi_many_f32(*args(16000, 1, nbytes.value - 1, None)) == -2
    assert lib.rtfs_debug_launch_count() == n0
    assert lib.rtfs_estoi_many_f32(*args(16000, 1, nbytes.value, None)) == 0  # ESTOI alone fits the plan's own workspace
    torch.cuda.synchronize()
    assert lib.rtfs_debug_launch_count() > n0 and (d == np.float32(0.0)).all()  # all-zero rows score exactly 0


def test_graph_capture_replays_eager():
    from rtfs_net_amd.metrics import estoi
    x, y = _case(4, 32000, 16000, 23, heavy_gap_rows=(2,))
    xd, yd = _dev(x), _dev(y)
    eager = estoi(xd, yd, return_kept=True, with_classic=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        estoi(xd, yd, with_classic=True)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = estoi(xd, yd, return_kept=True, with_classic=True)
    xd.copy_(_dev(x[::-1].copy()))  # new inputs in the captured buffers
    yd.copy_(_dev(y[::-1].copy()))
    g.replay()
    torch.cuda.synchronize()
    for o, e in zip(out, eager):
        assert torch.equal(o, e.flip(0))


# ---------------------------------------------------------------- 4. poisoned workspace and outputs
@pytest.mark.parametrize("byte", [0xFF, 0x7F], ids=["nan", "big"])
def test_poisoned_workspace_and_outputs(monkeypatch, byte):
    from rtfs_net_amd import _lib
    from rtfs_net_amd.metrics import estoi_many
    runs = [(_case(3, 32003, 16000, 30, heavy_gap_rows=(1,), zero_est_rows=(2,)), 16000), (_case(2, 4000, 16000, 31), 16000),
            (_case(3, 20001, 10000, 32, zero_clean_rows=(0,)), 10000)]
    edge = {J: xy for (L, J), xy in zip(E.SEGMENT_LENGTHS, segment_pool()[0]) if J in (18, 35, 257)}  # last planned chunk empty: 18, 35
    runs += [((x[None], y[None]), 10000) for x, y in edge.values()]
    cleans, ests = [_dev(x) for x, _ in segment_pool()[0]], [_dev(y) for _, y in segment_pool()[0]]

    def run():
        out = [_run(x, y, fs, with_classic=wc) for (x, y), fs in runs for wc in (False, True)]
        out.append(_host(*estoi_many(cleans, ests, 10000, return_kept=True)))
        out.append(_host(*estoi_many(cleans, ests, 10000, return_kept=True, with_classic=True)))
        return out

    clean = run()
    monkeypatch.setattr(_lib, "_POISON", byte)
    poisoned = run()  # _lib.check() verifies the guard band after the workspace of every call
    for a, b in zip(clean, poisoned):
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes() and np.isfinite(v).all()
    x, y = runs[0][0]
    _tracker_rows(x, y, True)  # the tracker's launches under poison too


# ---------------------------------------------------------------- 5. the tracker
def _tracker_rows(clean, est, estoi, fs=16000):
    import tempfile
    from rtfs_net_amd.metrics import ALLMetricsTracker
    rng = np.random.default_rng(40)
    mix = (clean + 0.8 * rng.standard_normal(clean.shape) * clean.std()).astype(np.float32)
    with tempfile.TemporaryDirectory() as td:
        t = ALLMetricsTracker(f"{td}/m.csv", fs=fs, estoi=estoi)
        t.update_batch(_dev(mix), _dev(clean[:, None]), _dev(est[:, None]), [f"k{b}" for b in range(clean.shape[0])])
        mean, std = t.get_mean(), t.get_std()
        t.final()
        rows = list(csv.DictReader(open(f"{td}/m.csv")))
    return mix, rows, mean, std


def _close(got, want):
    return abs(float(got) - float(want)) <= TOL * max(1.0, abs(float(want)))


def test_tracker_update_batch_with_estoi():
    x, y = _case(4, 32000, 16000, 41, heavy_gap_rows=(2,))
    mix, rows, mean, std = _tracker_rows(x, y, True)
    _, rows5, mean5, _ = _tracker_rows(x, y, False)
    assert list(rows[0]) == ["snt_id", "sdr", "sdr_i", "si-snr", "si-snr_i", "pesq", "stoi", "estoi"]
    assert [r["snt_id"] for r in rows] == [f"k{b}" for b in range(4)] + ["avg", "std"]
    want_e = []
    for b in range(4):
        sisnr, sisnr_i, sdr, sdr_i, st, est = E.tracker_values(mix[b], x[b:b + 1], y[b:b + 1])
        for k, v in {"sdr": sdr, "sdr_i": sdr_i, "si-snr": -sisnr, "si-snr_i": -sisnr_i, "stoi": st, "estoi": est}.items():
            assert _close(rows[b][k], v), (b, k, rows[b][k], v)
        want_e.append(est)
    for a, b in zip(rows5, rows):  # every reference column, the avg / std rows included, is text-identical: stoi bit-equal
        assert all(b[k] == v or (k == "pesq" and v == "nan") for k, v in a.items()), (a, b)
    assert _close(mean["estoi"], np.mean(want_e)) and _close(std["estoi"], np.std(want_e)) and mean["stoi"] == mean5["stoi"]
    assert _close(rows[4]["estoi"], np.mean(want_e)) and _close(rows[5]["estoi"], np.std(want_e))


def _tracker(tmp_path, name, feed, **kw):
    from rtfs_net_amd.metrics import ALLMetricsTracker
    t = ALLMetricsTracker(str(tmp_path / name), **kw)
    feed(t)
    mean, std = t.get_mean(), t.get_std()
    t.final()
    return list(csv.DictReader(open(tmp_path / name))), mean, std


def test_tracker_update_many_with_estoi(tmp_path):
    from tests.test_hip_score_many import on_device, pool
    recs, _ = pool(16000)
    mixes, cleans, ests = on_device(recs)
    keys = [f"utt{r}" for r in range(len(recs))]
    rows, mean, std = _tracker(tmp_path, "six.csv", lambda t: t.update_many(mixes, cleans, ests, keys), estoi=True)
    rows5 = _tracker(tmp_path, "five.csv", lambda t: t.update_many(mixes, cleans, ests, keys))[0]
    one = _tracker(tmp_path, "one.csv", lambda t: [t(m, c, e, k) for m, c, e, k in zip(mixes, cleans, ests, keys)], estoi=True)[0]
    assert [r["snt_id"] for r in rows] == keys + ["avg", "std"]
    want_e = []
    for r, (m, c, e) in enumerate(recs):
        est = E.estoi(c[0], e[0], 16000)
        assert _close(rows[r]["estoi"], est), (r, rows[r]["estoi"], est)
        assert rows[r]["estoi"] == one[r]["estoi"] and rows[r]["stoi"] == one[r]["stoi"]  # pooled and per-call: the same text
        want_e.append(float(rows[r]["estoi"]))
    for a, b in zip(rows5, rows):  # the reference columns do not notice the seventh
        assert all(b[k] == v or (k == "pesq" and v == "nan") for k, v in a.items()), (a, b)
    assert mean["estoi"] == np.mean(want_e) and std["estoi"] == np.std(want_e)


def test_system_evaluate_many_accepts_an_estoi_tracker(tmp_path):
    import rtfs_net_amd as R
    from oracle.params import make_inputs
    from tests.test_hip_longform import model
    from tests.test_hip_score_many import carve
    system = R.System(audio_model=model(4)).eval()
    rng = np.random.default_rng(400)
    wavs, embs, cleans = [], [], []
    for r, L in enumerate((8000, 20480)):
        wav, emb = make_inputs(1, L, -(-L // 640), 410 + r)
        wavs.append(carve(wav[0], r))
        embs.append(_dev(emb[0]))
        cleans.append(carve(M.speech_like(rng, L, 16000)[None], r + 1))
    kw = dict(window=16000, hop=6400)
    got = []
    rows = _tracker(tmp_path, "eval.csv", lambda t: got.extend(system.evaluate_many(wavs, cleans, embs, ["a", "b"], t, **kw)), estoi=True)[0]
    rows2 = _tracker(tmp_path, "upd.csv", lambda t: t.update_many(wavs, cleans, got, ["a", "b"]), estoi=True)[0]
    assert rows == rows2 and [r["snt_id"] for r in rows] == ["a", "b", "avg", "std"]
    for r, (c, g) in enumerate(zip(cleans, got)):
        want = E.estoi(c[0].cpu().numpy(), g[0].cpu().numpy(), 16000)
        assert np.isfinite(float(rows[r]["estoi"])) and _close(rows[r]["estoi"], want), (r, rows[r]["estoi"], want)
