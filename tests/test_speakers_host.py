"""Host side of the K-speaker separator (AVNet.separate_speakers, rtfs_separator_speakers_f32): workspace arithmetic, argument refusals
of the C entry and the Python shape checks - none of it touches a device."""
import copy
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ERR_ARG = -4


def lib():
    from rtfs_net_amd import _lib
    return _lib.load()


def test_speakers_workspace_arithmetic():
    L_ = lib()
    for B, L, Tv, split in [(1, 4096, 7, 0), (3, 5000, 9, 0), (16, 32000, 50, 2), (32, 32000, 50, 0), (1, 131072, 205, 0), (20, 8000, 12, 3)]:
        one = L_.rtfs_separator_speakers_workspace_bytes(B, 1, L, Tv, split)
        assert 0 < one <= L_.rtfs_separator_workspace_bytes_ex(B, L, Tv, split), (B, L, Tv, split)
        assert L_.rtfs_separator_speakers_workspace_bytes(B, 2, L, Tv, split) > one
    # 32 mixtures x 2 speakers at 2 s: less than the 64-row forward the replicated batch would take
    assert L_.rtfs_separator_speakers_workspace_bytes(32, 2, 32000, 50, 0) < L_.rtfs_separator_workspace_bytes_ex(64, 32000, 50, 0)
    for B, K, split in [(4, 0, 0), (4, 17, 0), (4, 2, 9), (0, 2, 0), (4, 2, -1)]:
        assert L_.rtfs_separator_speakers_workspace_bytes(B, K, 32000, 50, split) == 0, (B, K, split)


def test_speakers_entry_refuses_bad_arguments_before_any_device_call():
    L_ = lib()
    fake = ctypes.c_void_p(256)  # never dereferenced: every refusal below comes before the first device call
    ws = ctypes.c_void_p(4096)

    def call(K=2, repeats=4, wav=fake, out=fake, rnn_kind=0, split=0, B=1, L=32000):
        return L_.rtfs_separator_speakers_f32(wav, fake, fake, fake, fake, fake, fake, fake, out, B, K, L, 50, repeats, ws, 1 << 20, None, None,
                                              rnn_kind, split)

    assert call(K=0) == ERR_ARG
    assert call(K=17) == ERR_ARG
    assert call(repeats=1) == ERR_ARG
    assert call(wav=None) == ERR_ARG
    assert call(out=None) == ERR_ARG
    assert call(rnn_kind=2) == ERR_ARG
    assert call(split=9) == ERR_ARG
    assert call(B=0) == ERR_ARG
    assert call(L=128) == ERR_ARG


def _model():
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import RTFS4_AUDIONET
    return R.AVNet(print_macs=False, **copy.deepcopy(RTFS4_AUDIONET)).eval()


def test_separate_speakers_shape_errors_before_any_gpu_call():
    m = _model()
    wav = torch.zeros(2, 4096)
    with pytest.raises(ValueError):
        m.separate_speakers(wav, torch.zeros(3, 2, 512, 7))  # B mismatch
    with pytest.raises(ValueError):
        m.separate_speakers(wav, torch.zeros(2, 512, 7))  # (B,512,Tv): no speaker axis
    with pytest.raises(ValueError):
        m.separate_speakers(torch.zeros(2, 2, 4096), torch.zeros(2, 2, 512, 7))  # (B,2,L)
    with pytest.raises(ValueError):
        m.separate_speakers(torch.zeros(1, 2, 3, 4096), torch.zeros(1, 2, 512, 7))
    with pytest.raises(ValueError):
        m.separate_speakers(torch.zeros(4096), torch.zeros(2, 2, 512, 7))  # (L) is one mixture
    m.train()
    with pytest.raises(RuntimeError, match="inference only"):
        m.separate_speakers(wav, torch.zeros(2, 2, 512, 7))
    m.eval()
    with pytest.raises(RuntimeError, match="CPU tensor"):  # right shapes: the next check is the device
        m.separate_speakers(wav, torch.zeros(2, 2, 512, 7))


def test_system_separate_speakers_shape_error():
    import rtfs_net_amd as R
    s = R.System(audio_model=_model())
    with pytest.raises(ValueError):
        s.separate_speakers(torch.zeros(2, 4096), torch.zeros(2, 512))


def test_speakers_entry_refuses_the_exact_f32_switch():
    """RTFS_GEMM_F32=1 (read once per process: a child) runs the unfused A/B sequence, which has no shared prefix: -4 before any device call.
    (The 1-byte workspace would be refused next, with -2 and still before the device: without the switch the child prints -2.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import ctypes, sys; sys.path.insert(0, sys.argv[1]); from rtfs_net_amd import _lib; L = _lib.load(); f = ctypes.c_void_p(256); "
            "print(L.rtfs_separator_speakers_f32(f, f, f, f, f, f, f, f, f, 1, 2, 32000, 50, 4, f, 1, None, None, 0, 0))")
    pr = subprocess.run([sys.executable, "-c", code, root], env=dict(os.environ, RTFS_GEMM_F32="1"), capture_output=True, text=True, timeout=120)
    assert pr.returncode == 0, pr.stderr[-2000:]
    assert pr.stdout.strip().splitlines()[-1] == str(ERR_ARG), pr.stdout
