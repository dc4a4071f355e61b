"""GPU parity of the fused RTFS block, separator and VP block past 4 s of audio: the video block's long instance (121 <= Tv <= 256,
k_vp.hip), the fused block and separator up to T' = 512 with the SRU cell (8.2 s of audio) and the separator past 4 GB per tensor.
Inference bars (1e-4 max-rel, 1e-5 l2-rel) against the CPU oracle or the reference goldens, and library launch counts to show which
path ran (rtfs_debug_launch_count)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import rtfs_oracle as O
from oracle.params import make_inputs, make_state_dict
from tests.util import l2_rel, load_golden, rand, rel_err, spec_R4

pytestmark = pytest.mark.gpu

TOL = 1e-4
ERR_SHAPE = -1
SD = make_state_dict(spec_R4(), 0)
BLK = O._sub(SD, "refinement_module.audio_net.blocks")
VBLK = O._sub(SD, "refinement_module.video_net.blocks")
_M = {}


def model(repeats=4):
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import RTFS4_AUDIONET
    if repeats not in _M:
        c = copy.deepcopy(RTFS4_AUDIONET)
        c["audio_params"]["repeats"] = repeats
        m = R.AVNet(print_macs=False, **c)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in SD.items()})
        _M[repeats] = m.cuda().eval()
    return _M[repeats]


def lib():
    import rtfs_net_amd as R
    return R._lib.load()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def close(name, got, ref, tol=TOL, tol_l2=TOL / 10):
    e, l2 = rel_err(got, ref), l2_rel(got, ref)
    print(f"[long sep] {name}: max-rel {e:.3e}  l2-rel {l2:.3e}")
    assert np.isfinite(got).all(), name
    assert e <= tol and l2 <= tol_l2, f"{name}: max-rel {e:.3e} l2-rel {l2:.3e}"


def launches(fn):
    torch.cuda.synchronize()
    n0 = lib().rtfs_debug_launch_count()
    with torch.no_grad():
        y = fn()
    torch.cuda.synchronize()
    return y, lib().rtfs_debug_launch_count() - n0


# ---------------------------------------------------------------- 1. VP block
# 121: first frame past the short instance; 128 / 129: Lg 16 -> 17; 136: Lg 17; 205: 8.2 s at 25 fps; 249, 256: up to the maximum
@pytest.mark.parametrize("tv", [121, 128, 129, 136, 205, 249, 256])
def test_vp_block_long(tv):
    m = model()
    v = rand((2, 512, tv), 500 + tv)
    vd = dev(v)
    y, n = launches(lambda: m.refinement_module.video_net.blocks(vd))
    close(f"vp block Tv={tv}", host(y), O.vp_block(v, VBLK))
    assert n == 1, f"Tv={tv}: {n} launches (fused VP block: 1)"


def test_vp_block_past_256_stays_per_layer():
    m = model()
    v = rand((2, 512, 257), 757)
    vd = dev(v)
    y, n = launches(lambda: m.refinement_module.video_net.blocks(vd))
    close("vp block Tv=257 (per-layer)", host(y), O.vp_block(v, VBLK))
    assert n > 1, n


def test_vp_block_entry_point_205():
    from rtfs_net_amd import _lib
    m = model()
    L = lib()
    blk = m.refinement_module.video_net.get_block(0)
    v = rand((1, 512, 205), 905)
    x = dev(v)
    out = _lib.empty_like(x)
    pk = blk.pack_vp()
    torch.cuda.synchronize()
    rc = L.rtfs_vp_block_f32(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(pk.data_ptr()), ctypes.c_void_p(out.data_ptr()), 1, 205,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    close("rtfs_vp_block_f32 Tv=205", host(out), O.vp_block(v, VBLK))
    rc = L.rtfs_vp_block_f32(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(pk.data_ptr()), ctypes.c_void_p(out.data_ptr()), 1, 257,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == ERR_SHAPE, rc


# ---------------------------------------------------------------- 2. RTFS block
def _block(x, r=None):
    blocks = model().refinement_module.audio_net.blocks
    xd, rd = dev(x), None if r is None else dev(r)
    return launches(lambda: blocks(xd, rd))


# T' = 251 (first past the former cap), 256, 257 (second pass of the sweep), 400, 512 (8.2 s)
@pytest.mark.parametrize("T", [503, 513, 514, 801, 1025])
def test_rtfs_block_long(T):
    _, n250 = _block(rand((1, 256, 501, 129), 1501))  # the fused block at T' = 250: the count this path must not exceed
    x, r = rand((2, 256, T, 129), 600 + T), rand((2, 256, T, 129), 700 + T)
    ref = O.rtfs_block(np.concatenate([x + r, x[:1]]), BLK)  # (every norm is per sample: one oracle call for both GPU calls)
    y, n = _block(x, r)
    close(f"rtfs block(x + res) T={T} B=2", host(y), ref[:2])
    assert n <= n250, f"T={T}: {n} launches, the fused block at T' = 250 takes {n250}"
    y1, n1 = _block(x[:1])
    close(f"rtfs block T={T} B=1", host(y1), ref[2:])
    assert n1 <= n250, f"T={T}: {n1} launches, the fused block at T' = 250 takes {n250}"


def test_rtfs_block_past_512_stays_unfused():
    _, n250 = _block(rand((1, 256, 501, 129), 1501))
    x = rand((1, 256, 1027, 129), 1027)
    y, n = _block(x)
    close("rtfs block T=1027 (unfused)", host(y), O.rtfs_block(x, BLK))
    assert n > n250, (n, n250)


def _block_entry(T, rnn_kind):
    from rtfs_net_amd import _lib
    L = lib()
    blk = model().refinement_module.audio_net.get_block(0)
    x = torch.zeros(1, 256, T, 129, device="cuda")
    out = _lib.empty_like(x)
    ws = _lib.workspace(L.rtfs_block_workspace_bytes(1, T, 129), x.device)
    pk = blk.pack()
    rc = L.rtfs_block_f32(ctypes.c_void_p(x.data_ptr()), None, ctypes.c_void_p(pk.data_ptr()), ctypes.c_void_p(out.data_ptr()), 1, T, 129,
                          ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), rnn_kind)
    torch.cuda.synchronize()
    if rc == 0:
        _lib.check(rc, "rtfs_block_f32")  # under RTFS_POISON_WS: verifies the guard band after the workspace
        assert bool(torch.isfinite(out).all()), f"T={T}: non-finite block output"
    return rc


def test_rtfs_block_entry_point_limits():
    assert _block_entry(503, 1) == ERR_SHAPE  # LSTM cell: T' <= 250
    assert _block_entry(1027, 0) == ERR_SHAPE  # SRU cell: T' <= 512
    assert _block_entry(1025, 0) == 0


# ---------------------------------------------------------------- 3. whole model
def _golden_8s(B):
    wav, emb = make_inputs(1, 131072, 205, 34)  # the inputs of tests/golden/e2e_R4_L131072_B1 (oracle/make_golden_sizes.py)
    if B > 1:
        w2, e2 = make_inputs(B - 1, 131072, 205, 1034)
        wav, emb = np.concatenate([wav, w2]), np.concatenate([emb, e2])
    return wav, emb


@pytest.mark.parametrize("B", [1, 2])
def test_end_to_end_8s_vs_golden(B):
    m = model(4)
    wav, emb = _golden_8s(B)
    out = host(m(dev(wav), dev(emb)))
    assert out.shape == (B, 1, 131072)
    close(f"e2e 8.2 s B={B}, mixture 0 vs golden", out[:1], load_golden("e2e_R4_L131072_B1")["out"])


def test_launches_per_8s_forward():
    """A batch-1 8.2 s forward is the same launch chain as a short one (test_launches_per_small_batch_forward's window); the unfused path
    takes hundreds."""
    m = model(4)
    wav, emb = make_inputs(1, 131072, 205, 88)
    w, e = dev(wav), dev(emb)
    launches(lambda: m(w, e))
    _, n = launches(lambda: m(w, e))
    print(f"[launches] {n} per batch-1 8.2 s forward")
    assert 60 <= n <= 72, n


@pytest.mark.parametrize("L,Tv,seed", [(85000, 133, 41), (64000, 300, 42)], ids=["5.3s_ragged_Tv133", "4s_Tv300"])
def test_end_to_end_long_vs_oracle(L, Tv, seed):
    """5.3 s with an odd tail (T' = 332, long VP instance) and 4 s with 300 video frames (fused separator, per-layer VP block), R = 2."""
    m = model(2)
    wav, emb = make_inputs(1, L, Tv, seed)
    out = host(m(dev(wav), dev(emb)))
    close(f"e2e L={L} Tv={Tv} R=2", out, O.avnet_forward(wav, emb, SD, repeats=2))


# ---------------------------------------------------------------- 4. past 4 GB per tensor
def test_8s_batch_32_past_4gb():
    """8.2 s at B = 32: a full-resolution 256-channel tensor spans 4.3 GB (the workspace ~31 GB)."""
    m = model(4)
    try:
        wav, emb = _golden_8s(32)
        out = host(m(dev(wav), dev(emb)))
        assert out.shape == (32, 1, 131072) and np.isfinite(out).all()
        close("e2e 8.2 s B=32, mixture 0 vs golden", out[:1], load_golden("e2e_R4_L131072_B1")["out"])
        for i in (0, 1, 15, 16, 31):
            one = host(m(dev(wav[i:i + 1]), dev(emb[i:i + 1])))
            e = rel_err(out[i:i + 1], one)
            print(f"[long sep] B=32 mixture {i} vs alone: {e:.3e}")
            assert e <= 2e-6, f"mixture {i} differs from its batch-1 run by {e:.3e}"
    finally:
        torch.cuda.empty_cache()
