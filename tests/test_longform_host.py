"""Host side of long-form separation (AVNet.separate_long, rtfs_longform_plan): the plan arithmetic at its edges against
tests/longform_oracle.py, the partition of unity of the cross-fade, the edge replication of the video index, the refusals, and the public
method's CPU path against "oracle frame -> forward_modular per window -> oracle overlap-add".  None of it touches a device.

The package has no CPU arithmetic of its own (forward_modular on CPU tensors raises), so the CPU-path test gives a small RTFS-Net-2 a
``forward_modular`` that evaluates the model's own state dict with the numpy oracle of the reference forward (oracle/rtfs_oracle.py); both
sides of the comparison call it, the side under test in chunks, the expected side one window at a time."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import longform_oracle as LO

ERR_ARG = -4
SPF = 640


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


def c_plan(L, Tv, window, hop):
    n = ctypes.c_int(-1)
    rc = lib().rtfs_longform_plan(L, Tv, window, hop, ctypes.byref(n))
    return rc, n.value


def plans():
    """(L, window, hop) at the edges: L = window - 1, window, window + 1; L = window + k hop and +- 1; hop = window, window/2, window/4;
    hop = 640 with window = 1280."""
    out = []
    for window, hop in [(2560, 2560), (2560, 1280), (2560, 640), (1280, 640), (32000, 16000), (5120, 1920)]:
        for L in (window - 1, window, window + 1):
            out.append((L, window, hop))
        for k in (1, 2, 5):
            for d in (-1, 0, 1):
                out.append((window + k * hop + d, window, hop))
        out.append((7, window, hop))
    return out


def test_plan_arithmetic_at_the_edges():
    for L, window, hop in plans():
        rc, n = c_plan(L, 3, window, hop)
        want = LO.plan(L, 3, window, hop)
        assert rc == 0 and n == want, (L, window, hop, rc, n, want)
        # the last window reaches the end of the recording, the one before it does not
        assert (n - 1) * hop + window >= L
        assert n == 1 or (n - 2) * hop + window < L
    assert c_plan(32000 - 1, 50, 32000, 16000) == (0, 1)
    assert c_plan(32000, 50, 32000, 16000) == (0, 1)
    assert c_plan(32000 + 1, 50, 32000, 16000) == (0, 2)
    assert c_plan(32000 + 16000, 50, 32000, 16000) == (0, 2)
    assert c_plan(32000 + 16000 + 1, 50, 32000, 16000) == (0, 3)
    assert c_plan(300 * 16000, 7500, 32000, 16000) == (0, 299)
    assert lib().rtfs_longform_plan(48000, 75, 32000, 16000, None) == 0  # N may be NULL


def test_plan_refusals_agree_between_c_and_oracle():
    bad = [(48000, 75, 32001, 16000), (48000, 75, 32000, 16001), (48000, 75, 32000, 0), (48000, 75, 32000, -640), (48000, 75, 32000, 32640),
           (48000, 75, 0, 0), (0, 75, 32000, 16000), (48000, 0, 32000, 16000), (48000, 75, 1000, 500), (48000, 75, -640, -640)]
    for L, Tv, window, hop in bad:
        assert c_plan(L, Tv, window, hop)[0] == ERR_ARG, (L, Tv, window, hop)
        with pytest.raises(ValueError):
            LO.plan(L, Tv, window, hop)


def test_partition_of_unity():
    """An identity "model" (y_n = frame(x)_n): overlap_add gives x back to 1e-12 in float64, for every plan and two sources."""
    rng = np.random.default_rng(0)
    for L, window, hop in plans():
        x = rng.standard_normal((2, L))
        v = np.zeros((2, 512, 3))
        xw, _ = LO.frame(x, v, window, hop)
        assert xw.dtype == np.float64 and xw.shape == (2 * LO.plan(L, 3, window, hop), window)
        y = np.stack([xw, -2.0 * xw], axis=1)
        back = LO.overlap_add(y, 2, L, window, hop)
        assert back.shape == (2, 2, L)
        assert np.abs(back[:, 0] - x).max() <= 1e-12 and np.abs(back[:, 1] + 2.0 * x).max() <= 1e-12, (L, window, hop)
        w = LO.weights(window, hop)
        assert w.min() > 0 and w.max() <= 1.0 and np.array_equal(w, w[::-1])
    assert np.array_equal(LO.weights(2560, 2560), np.ones(2560))
    w = LO.weights(2560, 1280)
    assert w[0] == 0.5 / 1280 and w[1279] == 1279.5 / 1280 and w[1280] == 1279.5 / 1280
    w = LO.weights(2560, 1920)  # V = 640: ramps over the overlap, flat in between
    assert w[639] == 639.5 / 640 and np.all(w[640:1920] == 1.0) and w[1920] == 639.5 / 640


def test_small_cases_of_the_overlap_add():
    rng = np.random.default_rng(1)
    y = rng.standard_normal((1, 1, 2560))
    assert np.abs(LO.overlap_add(y, 1, 2000, 2560, 1280) - y[:, :, :2000]).max() <= 1e-15  # L <= window: the window cut to L
    y = rng.standard_normal((3, 1, 1280))
    assert np.array_equal(LO.overlap_add(y, 1, 3000, 1280, 1280), y.reshape(1, 1, 3840)[:, :, :3000])  # hop == window: concatenation


def test_video_index_edge_replication():
    for L, window, hop, Tv in [(12000, 5120, 2560, 19), (12000, 5120, 2560, 5), (12000, 5120, 2560, 40), (3000, 1280, 640, 1), (100, 1280, 640, 3)]:
        v = np.arange(2 * 512 * Tv, dtype=np.float64).reshape(2, 512, Tv)
        x = np.zeros((2, L))
        N = LO.plan(L, Tv, window, hop)
        _, vw = LO.frame(x, v, window, hop)
        assert vw.shape == (2 * N, 512, window // SPF)
        for b in range(2):
            for n in range(N):
                for f in range(window // SPF):
                    src = min(n * hop // SPF + f, Tv - 1)
                    assert np.array_equal(vw[b * N + n, :, f], v[b, :, src]), (b, n, f)


def test_torch_gathers_match_the_oracle():
    from rtfs_net_amd import models
    rng = np.random.default_rng(2)
    for L, window, hop in plans():
        if window > 5120:
            continue
        for Tv in (1, -(-L // SPF), 2 * -(-L // SPF) + 1):
            x, v = rng.standard_normal((2, L)).astype(np.float32), rng.standard_normal((2, 512, Tv)).astype(np.float32)
            N = LO.plan(L, Tv, window, hop)
            xw, vw = models._longform_frame_torch(torch.from_numpy(x), torch.from_numpy(v), N, window, hop)
            exw, evw = LO.frame(x, v, window, hop)
            assert np.array_equal(xw.numpy(), exw) and np.array_equal(vw.numpy(), evw), (L, window, hop, Tv)
            y = rng.standard_normal((2 * N, 2, window)).astype(np.float32)
            got = models._longform_overlap_add_torch(torch.from_numpy(y), 2, N, L, window, hop).numpy()
            want = LO.overlap_add(y, 2, L, window, hop)
            assert got.shape == want.shape and np.abs(got - want).max() <= 4 * -(-window // hop) * 2.0 ** -23 * np.abs(y).max()


def _model(repeats=2, cell="SRU"):
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import audionet_config
    return R.AVNet(print_macs=False, **copy.deepcopy(audionet_config(repeats, cell))).eval()


def test_separate_long_refusals():
    m = _model()
    wav, emb = torch.zeros(1, 48000), torch.zeros(1, 512, 75)
    for kw in (dict(window=32001), dict(hop=16001), dict(hop=0), dict(hop=-640), dict(window=32000, hop=32640), dict(window=0),
               dict(max_batch=0), dict(window=1000, hop=500)):
        with pytest.raises(ValueError):
            m.separate_long(wav, emb, **kw)
    with pytest.raises(ValueError):  # SRU cell: T/2 <= 512, i.e. windows up to 1024 * 128 samples + 127; the next multiple of 640 is past it
        m.separate_long(wav, emb, window=206 * 640)
    with pytest.raises(ValueError):  # LSTM cell: 4 s
        _model(2, "LSTM").separate_long(wav, emb, window=101 * 640)
    with pytest.raises(ValueError):  # GRU cell: no fused separator at all
        _model(2, "GRU").separate_long(wav, emb)
    with pytest.raises(ValueError):
        m.separate_long(torch.zeros(2, 2, 48000), torch.zeros(2, 512, 75))  # (B,2,L)
    with pytest.raises(ValueError):
        m.separate_long(wav, torch.zeros(2, 512, 75))  # B mismatch
    with pytest.raises(ValueError):
        m.separate_long(wav, torch.zeros(1, 75, 512))  # not (B,512,Tv)
    with pytest.raises(ValueError):
        m.separate_long(wav, None)
    with pytest.raises(ValueError):
        m.separate_long(wav, torch.zeros(1, 512, 0))  # no video frame to replicate
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        m.separate_long(wav, emb)
    m.eval()
    with pytest.raises(RuntimeError, match="CPU tensor"):  # right arguments: the CPU path reaches forward_modular, which has no CPU kernels
        m.separate_long(wav, emb)


def test_system_separate_long_forwards_its_arguments():
    import rtfs_net_amd as R
    s = R.System(audio_model=_model())
    with pytest.raises(ValueError):
        s.separate_long(torch.zeros(1, 48000), torch.zeros(1, 512, 75), window=32001)
    with pytest.raises(ValueError):
        s.separate_long(torch.zeros(1, 48000), torch.zeros(1, 512, 75), hop=100)


@pytest.mark.parametrize("L,Tv,max_batch", [(6000, 10, 3), (2560, 4, 32), (1400, 1, 32), (5121, 17, 2)])
def test_cpu_path_against_oracle_windows(L, Tv, max_batch):
    """separate_long on CPU tensors == oracle frame -> forward_modular per window -> oracle overlap-add (window 2560, hop 1280, B = 2: the
    shortest window whose coarsest time sweep still holds the dual-path kernel of 8)."""
    from oracle import rtfs_oracle as O
    from oracle.params import load_spec, make_inputs, make_state_dict
    m = _model(2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(load_spec("state_spec_R4.json"), 0).items()})
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    calls = []

    def forward_modular(wav, emb):
        calls.append(int(wav.shape[0]))  # row by row: a window's result must not depend on the chunk it arrives in
        rows = [O.avnet_forward(wav[i:i + 1].numpy(), emb[i:i + 1].numpy(), sd, repeats=2) for i in range(wav.shape[0])]
        return torch.from_numpy(np.concatenate(rows).astype(np.float32))

    m.forward_modular = forward_modular
    window, hop, B = 2560, 1280, 2
    wav, emb = make_inputs(B, L, Tv, 5)
    got = m.separate_long(torch.from_numpy(wav), torch.from_numpy(emb), window=window, hop=hop, max_batch=max_batch)
    N = LO.plan(L, Tv, window, hop)
    assert got.shape == (B, 1, L) and got.dtype == torch.float32
    chunks = list(calls)
    assert sum(chunks) == B * N and max(chunks) <= max_batch and len(chunks) == -(-B * N // max_batch), chunks
    xw, vw = LO.frame(wav, emb, window, hop)
    y = np.concatenate([forward_modular(torch.from_numpy(xw[i:i + 1]), torch.from_numpy(vw[i:i + 1])).numpy() for i in range(B * N)])
    want = LO.overlap_add(y, B, L, window, hop)
    err = float(np.abs(got.numpy() - want).max())
    # the windows are the same float32 values on both sides; then <= ceil(window / hop) float32 multiply-adds and a division per sample
    bound = 4 * -(-window // hop) * 2.0 ** -23 * np.abs(y).max()
    print(f"[longform host] L {L} Tv {Tv} N {N} chunks {chunks}: max abs err {err:.3e} (bound {bound:.3e}, max|y| {np.abs(y).max():.3e})")
    assert err <= bound, (err, bound)
    if L <= window:  # one window: forward on the zero-padded mixture, cut to L
        assert np.abs(got.numpy() - y[:, :, :L].reshape(B, 1, L)).max() <= 2.0 ** -22 * np.abs(y).max()
