"""GPU parity of the fused kernels past 4 s of audio: the SRU time sweep up to 512 positions (k_dualpath16s.hip, two passes of the four-part
workgroup) and the attention core up to 512 keys, against the CPU oracle at the inference bars (1e-4 max-rel, 1e-5 l2-rel)."""
import copy

import numpy as np
import pytest
import torch

from oracle import rtfs_oracle as O
from oracle.params import make_state_dict
from tests.util import l2_rel, rand, rel_err, spec_R4

pytestmark = pytest.mark.gpu

TOL = 1e-4
SD = make_state_dict(spec_R4(), 0)
BLK = O._sub(SD, "refinement_module.audio_net.blocks")
_M = []


def model():
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import RTFS4_AUDIONET
    if not _M:
        m = R.AVNet(print_macs=False, **copy.deepcopy(RTFS4_AUDIONET))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in SD.items()})
        _M.append(m.cuda().eval())
    return _M[0]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def close(name, got, ref):
    e, l2 = rel_err(got, ref), l2_rel(got, ref)
    print(f"[long] {name}: max-rel {e:.3e}  l2-rel {l2:.3e}")
    assert np.isfinite(got).all(), name
    assert e <= TOL and l2 <= TOL / 10, f"{name}: max-rel {e:.3e} l2-rel {l2:.3e}"


def launches(fn):
    import rtfs_net_amd as R
    lib = R._lib.load()
    torch.cuda.synchronize()
    n0 = lib.rtfs_debug_launch_count()
    y = fn()
    torch.cuda.synchronize()
    return y, lib.rtfs_debug_launch_count() - n0


# Sweep lengths Ls = L + 7 of the two-pass variant (257 <= Ls <= 512): L around the pass boundary (256), the time-part (64), tile (32), lane-half
# (16) and write-back group (4) boundaries of pass 1, the second row block of the load phase (Ls = 256 | 257) and the conv-transpose's second
# pass (Ls > 256), up to the longest sweep.
@pytest.mark.parametrize("Ls", [251, 256, 257, 258, 262, 263, 264, 266, 271, 279, 280, 287, 295, 296, 320, 327, 328, 359, 391, 392, 400, 455,
                                456, 487, 500, 505, 509, 511, 512])
def test_long_sweep_lengths(Ls):
    m = model()
    mod = m.refinement_module.audio_net.blocks.globalatt[1]
    x = rand((1, 64, Ls, 6), 900 + Ls)
    y, n = launches(lambda: mod(dev(x)))
    close(f"dualpath T sweep Ls={Ls}", host(y), O.dualpath_rnn(x, O._sub(BLK, "globalatt.1"), 3))
    assert n <= 4, f"{n} launches: the fused sweep is transpose + sweep + transpose"


@pytest.mark.parametrize("shape", [(1, 64, 512, 64), (2, 64, 333, 64)])
def test_long_sweep_full_rows(shape):
    m = model()
    x = rand(shape, 31 + shape[2])
    y, n = launches(lambda: m.refinement_module.audio_net.blocks.globalatt[1](dev(x)))
    close(f"dualpath T sweep {shape}", host(y), O.dualpath_rnn(x, O._sub(BLK, "globalatt.1"), 3))
    assert n <= 4, f"{n} launches: the fused sweep is transpose + sweep + transpose"


def test_long_sweep_span_sub_batches():
    """B = 520 at T = 512, F = 64: one (B,64,T,F) tensor spans 4.36 GB, past the sweep kernel's 32-bit offsets.  dualpath() runs it as
    sub-batches of 511 samples (< 4 GB each): two sweeps between the two transposes, and every sample equals its own batch-1 run - at the
    sub-batch boundary (510 | 511) as well."""
    B, T, F = 520, 512, 64
    per = 64 * T * F * 4
    nb = ((1 << 32) - 1) // per
    assert nb == 511 and B * per >= 1 << 32
    mod = model().refinement_module.audio_net.blocks.globalatt[1]
    g = torch.Generator(device="cuda").manual_seed(520)
    x = torch.randn((B, 64, T, F), generator=g, device="cuda")
    with torch.no_grad():
        y, n = launches(lambda: mod(x))
        assert n == 2 + -(-B // nb), f"{n} launches: transpose, one sweep per sub-batch, transpose"
        assert bool(torch.isfinite(y).all())
        for i in (0, 1, nb - 1, nb, B - 1):
            y1 = mod(x[i:i + 1].contiguous())
            d = float((y[i] - y1[0]).abs().max() / y1.abs().max())
            assert d <= 2e-6, f"sample {i}: {d:.3e} against its batch-1 run"
    del x, y
    torch.cuda.empty_cache()


def test_dualpath_sru_entry_point_400():
    """The C entry point itself takes a 400-position time sweep (it returned RTFS_ERR_SHAPE past 250)."""
    import rtfs_net_amd as R
    lib = R._lib.load()
    mod = model().refinement_module.audio_net.blocks.globalatt[1]
    B, T, F = 1, 400, 16
    xn = rand((B, 64, T, F), 4242)
    x = dev(xn)
    out = R._lib.empty_like(x)
    ws = R._lib.workspace(lib.rtfs_dualpath_workspace_bytes(B, T, F), x.device)
    rc = lib.rtfs_dualpath_sru_f32(R._lib.ptr(x), R._lib.ptr(mod.pack()), R._lib.ptr(out), B, T, F, 3, R._lib.ptr(ws), ws.numel(),
                                   R._lib.stream_of(x))
    assert rc == 0, rc
    R._lib.check(rc, "rtfs_dualpath_sru_f32")  # under RTFS_POISON_WS: verifies the guard band after the workspace
    close("rtfs_dualpath_sru_f32 T=400", host(out), O.dualpath_rnn(xn, O._sub(BLK, "globalatt.1"), 3))


def test_past_512_stays_unfused():
    """T' = 513: past the fused sweep, the unfused GEMM + scan + GEMM kernels (many launches)."""
    m = model()
    x = rand((1, 64, 513, 4), 513)
    y, n = launches(lambda: m.refinement_module.audio_net.blocks.globalatt[1](dev(x)))
    print(f"[long] T'=513: {n} launches")
    assert n > 4
    e = rel_err(host(y), O.dualpath_rnn(x, O._sub(BLK, "globalatt.1"), 3))
    assert e <= TOL, e


@pytest.mark.parametrize("T", [257, 384, 500, 512])
def test_long_attention(T):
    m = model()
    x = rand((1, 64, T, 64), 70 + T)
    y, n = launches(lambda: m.refinement_module.audio_net.blocks.globalatt[2](dev(x)))
    close(f"mhsa2d T={T}", host(y), O.mhsa2d(x, O._sub(BLK, "globalatt.2")))
    assert n <= 4, f"{n} launches: the fused attention is QKV rows + attention core + projection rows"


def test_past_512_keys_stays_unfused():
    """T = 513 keys: past the fused score tile, the batched-GEMM attention (many launches)."""
    m = model()
    x = rand((1, 64, 513, 64), 1513)
    y, n = launches(lambda: m.refinement_module.audio_net.blocks.globalatt[2](dev(x)))
    print(f"[long] T=513 keys: {n} launches")
    assert n > 4
    assert rel_err(host(y), O.mhsa2d(x, O._sub(BLK, "globalatt.2"))) <= TOL


def test_tf_attention_entry_point_384():
    """rtfs_tf_attention_f32 takes 384 keys (it returned RTFS_ERR_SHAPE past 256)."""
    import rtfs_net_amd as R
    lib = R._lib.load()
    mod = model().refinement_module.audio_net.blocks.globalatt[2]
    B, T = 2, 384
    xn = rand((B, 64, T, 64), 384)
    x = dev(xn)
    out = R._lib.empty_like(x)
    ws = R._lib.workspace(lib.rtfs_tf_attention_workspace_bytes(B, T), x.device)
    rc = lib.rtfs_tf_attention_f32(R._lib.ptr(x), R._lib.ptr(mod.pack()), R._lib.ptr(out), B, T, R._lib.ptr(ws), ws.numel(),
                                   R._lib.stream_of(x))
    assert rc == 0, rc
    R._lib.check(rc, "rtfs_tf_attention_f32")  # under RTFS_POISON_WS: verifies the guard band after the workspace
    close("rtfs_tf_attention_f32 T=384", host(out), O.mhsa2d(xn, O._sub(BLK, "globalatt.2")))
