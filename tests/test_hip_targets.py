"""A different number of target speakers per mixture with one audio pass (AVNet.separate_speakers(counts=...),
rtfs_separator_targets_f32, System.forward_grouped, AVNet.separate_many_speakers): target t must be what ``forward`` returns for the
mixture of target t with lips t.  The oracle is ``forward`` on the replicated batch, the bar the 2e-6 max-rel per target that
tests/test_hip_speakers.py holds the fixed-K call to (not bitwise: another batch composition); equal counts against the fixed-K call
and K all 1 against ``separate_many`` are bit for bit, because the table only replaces an index.  The forward cases run again in
child processes on poisoned memory (RTFS_POISON_WS)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.params import make_inputs
from tests.test_hip_speakers import BAR, dev, host, launches, model
from tests.util import l2_rel, load_golden, rel_err

pytestmark = pytest.mark.gpu

POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")


def tracks(N, Tv, seed):
    return np.random.RandomState(seed).randn(N, 512, Tv).astype(np.float32)


def vs_forward(name, m, counts, L, Tv, seed):
    """separate_speakers(counts=...) vs forward on the replicated rows; -> the ragged call's launch count."""
    B, N = len(counts), sum(counts)
    wav, _ = make_inputs(B, L, Tv, seed)
    w, e = dev(wav), dev(tracks(N, Tv, seed + 1))
    got, n = launches(lambda: m.separate_speakers(w, e, counts=counts))
    got = host(got)
    with torch.no_grad():
        ref = host(m(w.repeat_interleave(torch.tensor(counts).cuda(), 0), e))
    assert got.shape == (N, L), got.shape
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    worst = max(rel_err(got[t], ref[t, 0]) for t in range(N))
    print(f"[targets] {name}: worst per-target max-rel {worst:.3e} vs forward on {N} rows, {n} launches")
    assert worst <= BAR, f"{name}: {worst:.3e}"
    return n


# ---------------------------------------------------------------- 1. ragged separator vs forward on the replicated rows
def test_r4_sru_counts_1_3_2():
    vs_forward("R4 SRU counts [1,3,2] L5000", model(4), [1, 3, 2], 5000, 9, 31)


def test_two_repeats_one_boundary_first_and_last():
    vs_forward("R2 SRU counts [1,3,2] L5000", model(2), [1, 3, 2], 5000, 9, 32)


def test_lstm_counts_2_1():
    vs_forward("R4 LSTM counts [2,1] L4096", model(4, "LSTM"), [2, 1], 4096, 7, 33)


# ---------------------------------------------------------------- 2. reference anchor
def test_first_targets_vs_reference_golden():
    g = load_golden("e2e_R4_L5000_B3")
    wav, emb = make_inputs(3, 5000, 8, 3)
    counts, first = [2, 1, 3], [0, 2, 3]
    lp = tracks(6, 8, 34)
    lp[first] = emb  # the first target of each mixture: the golden input's lips
    out = host(model(4).separate_speakers(dev(wav), dev(lp), counts=counts))
    assert np.isfinite(out).all()
    for b, t in enumerate(first):
        e, l2 = rel_err(out[t], g["out"][b, 0]), l2_rel(out[t], g["out"][b, 0])
        print(f"[targets] e2e_R4_L5000_B3 mixture {b} target {t}: max-rel {e:.3e} l2-rel {l2:.3e}")
        assert e <= 1e-4 and l2 <= 1e-5, (b, e, l2)


# ---------------------------------------------------------------- 3. batch split
def test_batch_split_matches_unsplit():
    """16 mixtures, counts cycling 1,2,3 (31 targets): the second part starts at target 15 = sum(counts[:8]), which is 8 K for no K, and
    its kernels take mixture 8 as their base."""
    m = model(4)
    counts = [1 + b % 3 for b in range(16)]
    assert sum(counts[:8]) == 15 and sum(counts) == 31
    wav, _ = make_inputs(16, 4096, 7, 35)
    w, e = dev(wav), dev(tracks(sum(counts), 7, 36))
    ref = host(m.separate_speakers(w, e, counts=counts))
    m.batch_split = 2
    try:
        got = host(m.separate_speakers(w, e, counts=counts))
    finally:
        m.batch_split = 0
    worst = max(rel_err(got[t], ref[t]) for t in range(sum(counts)))
    print(f"[targets] split 2 vs unsplit: worst per-target max-rel {worst:.3e}")
    assert np.isfinite(got).all() and worst <= BAR, worst


# ---------------------------------------------------------------- 4. equal counts, launch count
def test_equal_counts_are_the_fixed_k_call():
    """Bit for bit: the same kernels, grids and operands, the table only replaces the division t / K.  (The fixed-K call repeated is
    printed beside it: the f64 atomics of the gLN statistics did not make two runs of one call differ either.)"""
    m = model(4)
    wav, _ = make_inputs(3, 5000, 9, 37)
    lp = tracks(6, 9, 38)
    w, e = dev(wav), dev(lp)
    got = host(m.separate_speakers(w, e, counts=[2, 2, 2]))
    ref = host(m.separate_speakers(w, e.view(3, 2, 512, 9))).reshape(6, 5000)
    again = host(m.separate_speakers(w, e.view(3, 2, 512, 9))).reshape(6, 5000)
    worst = max(rel_err(got[t], ref[t]) for t in range(6))
    print(f"[targets] counts [2,2,2] vs K = 2: bit-equal {np.array_equal(got, ref)}, worst max-rel {worst:.3e}; "
          f"K = 2 twice: bit-equal {np.array_equal(again, ref)}, max-rel {rel_err(again, ref):.3e}")
    assert np.array_equal(got, ref), worst


def test_b1_counts_2_launches_like_fixed_k2():
    m = model(4)
    wav, _ = make_inputs(1, 4096, 7, 77)
    w, lp = dev(wav), dev(tracks(2, 7, 78))
    m.separate_speakers(w, lp[None])
    m.separate_speakers(w, lp, counts=[2])
    _, n_fix = launches(lambda: m.separate_speakers(w, lp[None]))
    _, n_rag = launches(lambda: m.separate_speakers(w, lp, counts=[2]))
    print(f"[targets] launches: fixed K = 2 {n_fix}, counts [2] {n_rag}")
    assert n_rag == n_fix, (n_rag, n_fix)


# ---------------------------------------------------------------- 5. graph capture
def test_ragged_call_can_be_captured_in_a_hip_graph():
    m = model(4)
    counts = [1, 2]
    wav, _ = make_inputs(2, 8000, 12, 61)
    w, e = dev(wav), dev(tracks(3, 12, 62))
    ref = host(m.separate_speakers(w, e, counts=counts))  # (the table is cached from here on)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.separate_speakers(w, e, counts=counts)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.separate_speakers(w, e, counts=counts)
    g.replay()
    assert rel_err(host(out), ref) <= BAR
    wav2, _ = make_inputs(2, 8000, 12, 63)
    w.copy_(dev(wav2))
    e.copy_(dev(tracks(3, 12, 64)))
    g.replay()
    assert rel_err(host(out), host(m.separate_speakers(w, e, counts=counts))) <= BAR


# ---------------------------------------------------------------- 6. fallback routes
def test_gru_cell_composes_modules():
    n = vs_forward("R4 GRU counts [2,1] L4096", model(4, "GRU"), [2, 1], 4096, 7, 39)
    assert n > 200, n


def test_unfused_model_composes_inference_modules():
    m = model(4)
    m.fused = False
    try:
        vs_forward("R4 fused=False counts [1,2] L8000", m, [1, 2], 8000, 12, 40)
    finally:
        m.fused = True


# ---------------------------------------------------------------- 7. System.forward_grouped
def test_system_forward_grouped_runs_2_1_3():
    from oracle import video_oracle as V
    from tests.test_hip_speakers import _system
    s = _system()
    counts, L, Tv = [2, 1, 3], 8000, 12
    wav, _ = make_inputs(3, L, Tv, 41)
    w = dev(np.repeat(wav, counts, axis=0))
    mo = dev(V.make_video_input(6, Tv, 42))
    with torch.no_grad():
        ref = host(s(w, mo))
        _, n_fwd = launches(lambda: s(w, mo))
        got, n_grp = launches(lambda: s.forward_grouped(w, mo))
    got = host(got)
    assert got.shape == (6, 1, L)
    worst = max(rel_err(got[t], ref[t]) for t in range(6))
    print(f"[targets] forward_grouped runs 2,1,3: worst max-rel {worst:.3e}, {n_grp} launches, forward {n_fwd}")
    assert worst <= BAR, worst
    with torch.no_grad():  # System.separate_speakers with counts: the video model once on the 6 tracks
        sp = host(s.separate_speakers(dev(wav), mo, counts=counts))
    assert max(rel_err(sp[t], ref[t, 0]) for t in range(6)) <= BAR


# ---------------------------------------------------------------- 8. pooled recordings with faces
MANY = dict(window=6400, hop=3200, max_batch=5)
MANY_L, MANY_K = [1, 6400, 10001, 20000], [2, 1, 3, 1]


def _many_inputs(seed):
    rng = np.random.RandomState(seed)
    wavs = [dev((0.1 * rng.randn(L)).astype(np.float32)) for L in MANY_L]
    lips = [dev(rng.randn(K, 512, max(1, -(-L // 640) + r - 1)).astype(np.float32)) for r, (L, K) in enumerate(zip(MANY_L, MANY_K))]
    return wavs, lips


def test_frame_many_speakers_kernel_is_a_copy():
    """The framing launch against the torch gather, bit for bit: each audio window once, its K_r video windows at trow0 + n K_r + k."""
    import ctypes
    from rtfs_net_amd import _lib as L_
    from rtfs_net_amd.models import _longform_frame_torch
    from tests import targets_oracle as TO
    wavs, lips = _many_inputs(50)
    window, hop, R = 6400, 3200, 4
    p = TO.plan(MANY_L, [int(v.shape[2]) for v in lips], MANY_K, window, hop)
    arr = lambda v: (ctypes.c_longlong * R)(*v)
    table = (ctypes.c_longlong * (7 * R))()
    assert L_.load().rtfs_longform_many_speakers_plan(arr(p["L"]), arr(p["Tv"]), arr(p["K"]), R, window, hop, table, None, None, None) == 0
    assert list(table) == TO.table(p)
    tab = torch.tensor(list(table) + [w.data_ptr() for w in wavs] + [v.data_ptr() for v in lips], dtype=torch.int64).cuda()
    xw = L_.empty(p["rows"], window, device=tab.device)
    vw = L_.empty(p["targets"], 512, window // 640, device=tab.device)
    L_.check(L_.load().rtfs_longform_frame_many_speakers_f32(L_.ptr(tab[7 * R:8 * R]), L_.ptr(tab[8 * R:]), L_.ptr(tab), L_.ptr(xw), L_.ptr(vw),
                                                             R, p["rows"], max(MANY_K), window, hop, L_.stream_of(xw)), "frame_many_speakers")
    for r in range(R):
        a, v = _longform_frame_torch(wavs[r][None], lips[r].reshape(1, -1, lips[r].shape[2]), p["N"][r], window, hop)
        assert torch.equal(xw[p["row0"][r]:p["row0"][r] + p["N"][r]], a), r
        assert torch.equal(vw[p["trow0"][r]:p["trow0"][r] + p["N"][r] * MANY_K[r]], v.reshape(-1, 512, window // 640)), r


def test_separate_many_speakers_vs_separate_many_per_face():
    """Lengths 1, 6400, 10001, 20000 with K = 2,1,3,1 in windows of 6400 every 3200 (1, 1, 3, 6 windows: 2, 1, 9, 6 targets), at most 5
    targets a chunk: chunks straddle recordings and one closes in the middle of recording 2."""
    m = model(4)
    wavs, lips = _many_inputs(51)
    with torch.no_grad():
        got = m.separate_many_speakers(wavs, lips, **MANY)
        worst = 0.0
        for r in range(4):
            assert tuple(got[r].shape) == (MANY_K[r], MANY_L[r])
            for k in range(MANY_K[r]):
                ref = host(m.separate_many([wavs[r]], [lips[r][k]], window=6400, hop=3200)[0][0])
                g = host(got[r][k])
                assert np.isfinite(g).all()
                e = rel_err(g, ref)
                print(f"[targets] many: recording {r} (L {MANY_L[r]}) face {k}: max-rel {e:.3e}")
                worst = max(worst, e)
    assert worst <= BAR, worst


def test_separate_many_speakers_with_one_face_each_is_separate_many():
    """K all 1 against ``separate_many``, bit for bit: the same windows in the same chunks, and a table that maps target t to mixture t."""
    m = model(4)
    wavs, lips = _many_inputs(52)
    with torch.no_grad():
        got = m.separate_many_speakers(wavs, [lp[:1] for lp in lips], **MANY)
        ref = m.separate_many(wavs, [lp[0] for lp in lips], **MANY)
    worst = max(rel_err(host(a), host(b)) for a, b in zip(got, ref))
    print(f"[targets] many, one face each vs separate_many: bit-equal {all(torch.equal(a, b) for a, b in zip(got, ref))}, max-rel {worst:.3e}")
    assert all(torch.equal(a, b) for a, b in zip(got, ref)), worst


# ---------------------------------------------------------------- 9. refusals
def test_refusals():
    m = model(4)
    w = dev(make_inputs(2, 4096, 7, 0)[0])
    for counts, n in (([1, 2, 1], 4), ([1, 2], 4), ([0, 3], 3), ([17, 1], 18)):
        with pytest.raises(ValueError):
            m.separate_speakers(w, dev(tracks(n, 7, 0)), counts=counts)
    with pytest.raises(ValueError):
        m.separate_many_speakers([w[0]], [dev(tracks(17, 7, 0))])
    with pytest.raises(ValueError):
        m.separate_many_speakers([w[0]], [dev(tracks(2, 7, 0))[0]])
    m.train()
    try:
        with pytest.raises(RuntimeError):
            m.separate_speakers(w, dev(tracks(3, 7, 0)), counts=[1, 2])
    finally:
        m.eval()


# ---------------------------------------------------------------- 10. poisoned memory
FORWARD_CASES = ("test_r4_sru or test_two_repeats or test_lstm or test_first_targets or test_batch_split or test_equal_counts or "
                 "test_unfused or test_system or test_frame_many or test_separate_many")


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
@pytest.mark.parametrize("pattern", ["nan", "big"])
def test_poisoned(pattern):
    """This file's forward cases in a fresh child process with every workspace / output poisoned (tests/test_hip_poisoned.py's pattern)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RTFS_POISON_WS=pattern)
    try:
        pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_targets.py"), "-m", "gpu", "-q", "-p",
                             "no:cacheprovider", "-k", FORWARD_CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s")
    assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
