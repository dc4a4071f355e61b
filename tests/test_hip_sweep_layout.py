"""GPU parity of the RTFS block's channel-last route: the frequency sweep writes (B, T', F', 64) rows, the time sweep reads and writes them and
the attention reads them, with no transposes (api.hip block_body, k_dualpath16s.hip layouts 2 and 3, k_attn.hip row_can_kernel<., true>).
The module-level block ABI against the CPU oracle at the inference bars (1e-4 max-rel, 1e-5 l2-rel) over time lengths that cross the tile,
part and pass boundaries of every sweep variant, and the block's launch count on both routes (RTFS_SWEEP_GEN2=1 keeps the channel-major
sequence with its two transposes; it is re-run in a child process because the switch is read once per process)."""
import copy
import os

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
GEN2 = bool(os.environ.get("RTFS_SWEEP_GEN2"))
_M = []


def blocks():
    import rtfs_net_amd as R
    from rtfs_net_amd.configs import RTFS4_AUDIONET
    if not _M:
        m = R.AVNet(print_macs=False, **copy.deepcopy(RTFS4_AUDIONET))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in SD.items()})
        _M.append(m.cuda().eval())
    return _M[0].refinement_module.audio_net.blocks


def launches(fn):
    import rtfs_net_amd as R
    lib = R._lib.load()
    torch.cuda.synchronize()
    n0 = lib.rtfs_debug_launch_count()
    y = fn()
    torch.cuda.synchronize()
    return y, lib.rtfs_debug_launch_count() - n0


def close(name, got, ref):
    e, l2 = rel_err(got, ref), l2_rel(got, ref)
    print(f"[layout] {name}: max-rel {e:.3e}  l2-rel {l2:.3e}")
    assert np.isfinite(got).all(), name
    assert e <= TOL and l2 <= TOL / 10, f"{name}: max-rel {e:.3e} l2-rel {l2:.3e}"


# T' = T // 2 (F = 129: F' = 64).  Paired variant (Ls <= 64): 8, 57, 63, 64; 2 s variant (65 .. 128): 65, 71, 125, 128; four-part variant
# (129 .. 256): 129, 135, 250, 256; two-pass variant (257 .. 512): 257, 300, 512.  Odd batches: 3 up to T' = 135, 1 past it.
@pytest.mark.parametrize("Tp", [8, 57, 63, 64, 65, 71, 125, 128, 129, 135, 250, 256, 257, 300, 512])
def test_block_channel_last_route(Tp):
    B = 3 if Tp <= 135 else 1
    T = 2 * Tp + (Tp & 1)  # (odd T for odd T': the dropped last row)
    x = rand((B, 256, T, 129), 9100 + Tp)
    y = blocks()(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    close(f"rtfs block T'={Tp} B={B}{' (gen2)' if GEN2 else ''}", y.cpu().numpy(), O.rtfs_block(x, BLK))


def test_block_launch_count():
    """Head + 13 body launches + tail.  The channel-major route takes two more: the transposes around the time sweep."""
    x = torch.from_numpy(rand((1, 256, 250, 129), 9001)).cuda()
    blk = blocks()
    launches(lambda: blk(x))
    _, n = launches(lambda: blk(x))
    print(f"[layout] {n} launches per block application{' (gen2)' if GEN2 else ''}")
    assert n == (17 if GEN2 else 15), n


def test_channel_major_route_still_passes():
    """RTFS_SWEEP_GEN2=1: the block runs today's channel-major sequence (generation-2 sweeps, two transposes) at T' <= 256."""
    import subprocess
    import sys
    if GEN2:
        pytest.skip("already inside the generation-2 run")
    env = dict(os.environ, RTFS_SWEEP_GEN2="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pr = subprocess.run([sys.executable, "-m", "pytest", "tests/test_hip_sweep_layout.py", "-q", "-x", "-m", "gpu", "-k",
                         "test_block_launch_count or test_block_channel_last_route[57] or test_block_channel_last_route[125] or "
                         "test_block_channel_last_route[250]"],
                        cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert pr.returncode == 0, pr.stdout[-3000:]
