"""The GPU suite again with poisoned memory: every workspace, every output and every saved-for-backward tensor a C call fills starts
out as the poison byte (rtfs-net_amd/_lib.py: RTFS_POISON_WS), and each workspace is followed by a poisoned guard band that
_lib.check() verifies after the call.

A kernel that reads a byte its call did not write, or leaves an output element unwritten, otherwise reads whatever torch's caching
allocator left in that block, often the same tensor of the previous call at the same shape, and then the stale value is exactly the
right one.  Two patterns:

* ``nan`` (0xFF bytes: NaN as f32 and f64) turns such a read into NaN in the compared output, and any element a kernel skips;
* ``big`` (0x7F bytes: 3.4e38 as f32) is finite, so it also survives the fmaxf of a ReLU / max-pool epilogue or the STFT's per-tile
  scale, where a NaN operand silently disappears, and turns into inf or a huge error downstream.

Each (pattern, file) runs in a fresh child process.  A child that ends by a signal, a time limit, an abort or a segmentation fault
may have left the card faulted: the children after it are not started.
"""
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

if os.environ.get("RTFS_POISON_WS", "") not in ("", "0"):
    pytest.skip("already inside a poisoned run", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORWARD = ["test_hip_parity.py", "test_hip_sweep_layout.py", "test_hip_long.py", "test_hip_long_separator.py", "test_hip_sizes.py",
           "test_hip_dw_edges.py", "test_hip_pw_edges.py", "test_hip_attn_edges.py"]
# (test_hip_nearest.py: forward and training cases in one file; its forward cases also run on both patterns in-process)
TRAINING = ["test_hip_training.py", "test_hip_training_full.py", "test_hip_training_edges.py", "test_hip_training_conv_edges.py",
            "test_hip_nearest.py"]
# unpoisoned wall time of each file as one child on an MI355X (s; test_hip_training_full.py: its pytest time); the child's limit is
# about three times that, and at least two minutes
WALL_S = {"test_hip_parity.py": 48, "test_hip_sweep_layout.py": 41, "test_hip_long.py": 9, "test_hip_long_separator.py": 53,
          "test_hip_sizes.py": 17, "test_hip_training.py": 28, "test_hip_training_full.py": 190, "test_hip_training_edges.py": 110, "test_hip_training_conv_edges.py": 12, "test_hip_nearest.py": 10, "test_hip_dw_edges.py": 10, "test_hip_pw_edges.py": 26,
          "test_hip_attn_edges.py": 47}
CHILDREN = [("nan", f) for f in FORWARD + TRAINING] + [("big", f) for f in FORWARD]
ABNORMAL = (124, 134, 137, 139)
_stopped = []  # the child that ended abnormally, if one did


@pytest.mark.parametrize("pattern,name", CHILDREN, ids=[f"{p}-{f[:-3]}" for p, f in CHILDREN])
def test_poisoned(pattern, name):
    if _stopped:
        pytest.fail(f"not run: an earlier poisoned child ended abnormally ({_stopped[0]})")
    env = dict(os.environ, RTFS_POISON_WS=pattern)
    limit = max(120, 3 * WALL_S[name])
    t0 = time.monotonic()
    try:
        pr = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", name), "-m", "gpu", "-q", "-p", "no:cacheprovider"],
                            cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        _stopped.append(f"{pattern} {name}: timed out after {limit} s")
        out = (e.stdout or b"")
        out = out.decode(errors="replace") if isinstance(out, bytes) else out
        pytest.fail(f"RTFS_POISON_WS={pattern} {name}: timed out after {limit} s\n{out[-3000:]}")
    wall = time.monotonic() - t0
    print(f"RTFS_POISON_WS={pattern} {name}: rc {pr.returncode}, {wall:.0f} s")
    if pr.returncode < 0 or pr.returncode in ABNORMAL:
        _stopped.append(f"{pattern} {name}: exit status {pr.returncode}")
    assert pr.returncode == 0, f"RTFS_POISON_WS={pattern} {name}: exit status {pr.returncode} after {wall:.0f} s\n" \
                               f"{pr.stdout[-3000:]}\n{pr.stderr[-2000:]}"
