"""K target speakers of one mixture with one audio pass (AVNet.separate_speakers, rtfs_separator_speakers_f32, System.separate_speakers /
forward_grouped): target k of mixture b must be what ``forward`` returns for that mixture with lips k - against the reference's golden vectors
for speaker 0, and against ``forward`` on the replicated batch for every target (<= 2e-6 max-rel: the suite's batch-vs-batch bar; not
bitwise, the gLN statistics are f64 atomics).  The forward cases run again in child processes on poisoned memory (RTFS_POISON_WS)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.params import make_inputs, make_state_dict
from tests.util import l2_rel, load_golden, rel_err, spec_R4

pytestmark = pytest.mark.gpu

BAR = 2e-6
POISONED = os.environ.get("RTFS_POISON_WS", "") not in ("", "0")
_MODELS = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def model(repeats=4, cell="SRU"):
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import audionet_config
    key = (repeats, cell)
    if key not in _MODELS:
        torch.manual_seed(7)  # (the GRU cell has no spec file: torch's own initialisation, seeded)
        m = R.AVNet(print_macs=False, **audionet_config(repeats, cell))
        if cell == "SRU":
            sd = make_state_dict(spec_R4(), 0)
        elif cell == "LSTM":
            import json
            from tests.util import GOLDEN
            sd = make_state_dict(json.load(open(os.path.join(GOLDEN, "state_spec_R4_lstm.json"))), 0)
        else:
            sd = None
        if sd is not None:
            m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        _MODELS[key] = m.cuda().eval()
    return _MODELS[key]


def lips(B, K, Tv, seed):
    return np.random.RandomState(seed).randn(B, K, 512, Tv).astype(np.float32)


def launches(fn):
    from rtfs_net_amd import _lib
    torch.cuda.synchronize()
    n0 = _lib.load().rtfs_debug_launch_count()
    with torch.no_grad():
        y = fn()
    torch.cuda.synchronize()
    return y, _lib.load().rtfs_debug_launch_count() - n0


def vs_forward(name, m, B, K, L, Tv, seed):
    """separate_speakers on (B mixtures, K lips each) vs forward on the replicated batch; returns the separate_speakers launch count."""
    wav, _ = make_inputs(B, L, Tv, seed)
    lp = lips(B, K, Tv, seed + 1)
    w, e = dev(wav), dev(lp)
    got, n = launches(lambda: m.separate_speakers(w, e))
    got = host(got)
    with torch.no_grad():
        ref = host(m(w.repeat_interleave(K, 0), e.reshape(B * K, 512, Tv)))
    assert got.shape == (B, K, L), got.shape
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    worst = max(rel_err(got[b, k], ref[b * K + k, 0]) for b in range(B) for k in range(K))
    print(f"[speakers] {name}: worst per-target max-rel {worst:.3e} vs forward on {B * K} rows, {n} launches")
    assert worst <= BAR, f"{name}: {worst:.3e}"
    return n


# ---------------------------------------------------------------- 1. reference anchor
@pytest.mark.parametrize("cell,name", [("SRU", "e2e_R4_L32000_B1"), ("LSTM", "e2e_lstm_R4_L32000_B1")])
def test_speaker0_vs_reference_golden(cell, name):
    g = load_golden(name)
    wav, emb = make_inputs(1, 32000, 50, 2)
    lp = np.concatenate([emb[:, None], lips(1, 1, 50, 5)], axis=1)  # speaker 0: the golden input's lips; speaker 1: another track
    out = host(model(4, cell).separate_speakers(dev(wav), dev(lp)))
    e, l2 = rel_err(out[:, :1], g["out"]), l2_rel(out[:, :1], g["out"])
    print(f"[speakers] {name} speaker 0: max-rel {e:.3e} l2-rel {l2:.3e}")
    assert np.isfinite(out).all() and e <= 1e-4 and l2 <= 1e-5, (e, l2)


# ---------------------------------------------------------------- 2. every target vs forward on the replicated batch
@pytest.mark.parametrize("cell", ["SRU", "LSTM"])
def test_r4_b32_k2_2s(cell):
    vs_forward(f"R4 {cell} B32 K2 2s", model(4, cell), 32, 2, 32000, 50, 11)


def test_r12_b8_k2_4s():
    vs_forward("R12 B8 K2 4s", model(12), 8, 2, 64000, 100, 12)


def test_b3_k3_odd_length():
    vs_forward("R4 B3 K3 L5000", model(4), 3, 3, 5000, 9, 13)


def test_b1_k2_longest_fused():
    vs_forward("R4 B1 K2 8.2 s (T' = 512)", model(4), 1, 2, 1024 * 128, 205, 14)


def test_k1_is_forward():
    vs_forward("R4 B4 K1", model(4), 4, 1, 8000, 12, 15)


# ---------------------------------------------------------------- 3 + 4. fallback routes, launch counts
def test_gru_cell_composes_modules():
    n = vs_forward("R4 GRU B2 K2 L4096", model(4, "GRU"), 2, 2, 4096, 7, 16)
    assert n > 200, n


def test_one_frame_past_the_fused_limit_composes_modules():
    n = vs_forward("R4 SRU B1 K2 T/2 = 513", model(4), 1, 2, 1025 * 128, 206, 17)
    assert n > 200, n


def test_unfused_model_composes_inference_modules():
    """fused = False: the per-module inference entry points (encoder statistics handed to the bottleneck), as forward_modular."""
    m = model(4)
    m.fused = False
    try:
        vs_forward("R4 fused=False B2 K2 L8000", m, 2, 2, 8000, 12, 26)
    finally:
        m.fused = True


def test_fused_b1_k2_launches_like_a_batch1_forward():
    m = model(4)
    wav, emb = make_inputs(1, 4096, 7, 77)
    w, e = dev(wav), dev(emb)
    lp = dev(lips(1, 2, 7, 78))
    m(w, e)
    m.separate_speakers(w, lp)
    _, n_fwd = launches(lambda: m(w, e))
    _, n_spk = launches(lambda: m.separate_speakers(w, lp))
    print(f"[speakers] launches: batch-1 forward {n_fwd}, B = 1 K = 2 {n_spk}")
    assert n_spk == n_fwd, (n_spk, n_fwd)


# ---------------------------------------------------------------- 5. batch split
def test_batch_split_matches_unsplit():
    m = model(4)
    B, K, L, Tv = 16, 2, 8000, 12
    wav, _ = make_inputs(B, L, Tv, 18)
    w, e = dev(wav), dev(lips(B, K, Tv, 19))
    ref = host(m.separate_speakers(w, e))
    m.batch_split = 2
    try:
        got = host(m.separate_speakers(w, e))
    finally:
        m.batch_split = 0
    assert rel_err(got, ref) <= BAR, rel_err(got, ref)


# ---------------------------------------------------------------- 6. graph capture
def test_separate_speakers_can_be_captured_in_a_hip_graph():
    m = model(4)
    wav, _ = make_inputs(2, 8000, 12, 61)
    w, e = dev(wav), dev(lips(2, 2, 12, 62))
    ref = host(m.separate_speakers(w, e))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.separate_speakers(w, e)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.separate_speakers(w, e)
    g.replay()
    assert rel_err(host(out), ref) <= BAR
    wav2, _ = make_inputs(2, 8000, 12, 63)
    w.copy_(dev(wav2))
    e.copy_(dev(lips(2, 2, 12, 64)))
    g.replay()
    assert rel_err(host(out), host(m.separate_speakers(w, e))) <= BAR


# ---------------------------------------------------------------- 8. System
def _system():
    import rtfs_net_amd as R
    from oracle import video_oracle as V
    if "sys" not in _MODELS:
        video = R.FRCNNVideoModel(print_macs=False)
        video.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in V.make_video_state_dict(0).items()})
        _MODELS["sys"] = R.System(audio_model=model(4), video_model=video.cuda().eval()).eval()
    return _MODELS["sys"]


def test_system_separate_speakers_vs_forward():
    from oracle import video_oracle as V
    s = _system()
    B, K, L, Tv = 2, 2, 8000, 12
    wav, _ = make_inputs(B, L, Tv, 20)
    mouths = V.make_video_input(B * K, Tv, 21).reshape(B, K, 1, Tv, 88, 88)
    w, mo = dev(wav), dev(mouths)
    got = host(s.separate_speakers(w, mo))
    with torch.no_grad():
        ref = host(s(w.repeat_interleave(K, 0), mo.reshape(B * K, 1, Tv, 88, 88)))
    assert got.shape == (B, K, L)
    assert rel_err(got.reshape(B * K, 1, L), ref) <= BAR, rel_err(got.reshape(B * K, 1, L), ref)


def test_system_forward_grouped_on_a_test_layout_batch():
    """The reference's test batch (test.py:128-140): 4 mixtures x 2 target speakers, each mixture's rows side by side."""
    from oracle import video_oracle as V
    s = _system()
    M, K, L, Tv = 4, 2, 32000, 50
    wav, _ = make_inputs(M, L, Tv, 22)
    w = dev(np.repeat(wav, K, axis=0))
    mo = dev(V.make_video_input(M * K, Tv, 23))
    with torch.no_grad():
        ref = host(s(w, mo))
        _, n_fwd = launches(lambda: s(w, mo))
        got, n_grp = launches(lambda: s.forward_grouped(w, mo))
    got = host(got)
    assert got.shape == (M * K, 1, L)
    assert rel_err(got, ref) <= BAR, rel_err(got, ref)
    print(f"[speakers] forward_grouped: {n_grp} launches, forward {n_fwd}")


def test_system_forward_grouped_without_repeats_is_forward():
    from oracle import video_oracle as V
    s = _system()
    N, L, Tv = 4, 8000, 12
    wav, _ = make_inputs(N, L, Tv, 24)
    wav[2] = wav[1]  # one pair, the rest single: runs of unequal length -> forward
    w, mo = dev(wav), dev(V.make_video_input(N, Tv, 25))
    with torch.no_grad():
        ref = host(s(w, mo))
        got = host(s.forward_grouped(w, mo))
    assert rel_err(got, ref) <= BAR


# ---------------------------------------------------------------- 9. refusals
def test_refusals():
    m = model(4)
    w = dev(make_inputs(2, 4096, 7, 0)[0])
    with pytest.raises(ValueError):
        m.separate_speakers(w, dev(lips(3, 2, 7, 0)))
    m.train()
    try:
        with pytest.raises(RuntimeError):
            m.separate_speakers(w, dev(lips(2, 2, 7, 0)))
    finally:
        m.eval()


# ---------------------------------------------------------------- 7. poisoned memory
FORWARD_CASES = ("test_speaker0 or test_r4_b32 or test_r12 or test_b3 or test_b1_k2 or test_k1 or test_batch_split or test_system or "
                 "test_unfused")


@pytest.mark.skipif(POISONED, reason="already inside a poisoned run")
@pytest.mark.parametrize("pattern", ["nan", "big"])
def test_poisoned(pattern):
    """This file's forward cases in a fresh child process with every workspace / output poisoned (tests/test_hip_poisoned.py's pattern)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RTFS_POISON_WS=pattern)
    try:
        pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hip_speakers.py"), "-m", "gpu", "-q", "-p",
                             "no:cacheprovider", "-k", FORWARD_CASES], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.fail(f"RTFS_POISON_WS={pattern}: timed out after 300 s")
    assert pr.returncode == 0, f"RTFS_POISON_WS={pattern}: exit status {pr.returncode}\n{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
