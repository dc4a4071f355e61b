"""GPU: the video front-end (csrc/k_video.hip) and the short instance of the fused VP block (csrc/k_vp.hip) against float64 at the
frame counts where their tiling changes behaviour.

vid_conv_kernel flattens N * Ho * Wo output pixels into 128-pixel tiles and lays its grid out in rounds of 8 pixel tiles x ncb
output-channel blocks (slot = blockIdx.x >> 3, ptile = (slot / ncb) * 8 + (blockIdx.x & 7), cb = slot % ncb).  A stage leaves its
first round once N * Ho * Wo > 1024:

    stage                  pixels / frame   ncb   second round at
    stem (44 x 44)         1936             1     N >= 1
    layer 1 (22 x 22)      484              1     (LDS kernel: per-frame grid, two row bands per frame)
    layer 2 (11 x 11)      121              1     N >= 9
    layer 3 (6 x 6)        36               2     N >= 29
    layer 4 (3 x 3)        9                4     N >= 114, third round at N >= 228

The numpy oracle takes a second per frame, so the reference here is oracle/video_ref64.py (float64 torch ops, pinned on the CPU against
the numpy oracle and the reference module's outputs in tests/test_oracle_golden.py).  Bars: the project's inference bars (1e-4 max-rel,
1e-5 l2-rel) and the same 1e-4 per frame (tests/util.frame_rel_err), which a wrong low-magnitude frame cannot hide behind.

Every call runs on poisoned scratch and output, once per pattern: 0xFF (NaN) and 0x7F (3.4e38: finite, so it survives the fmaxf of the
max pool); a run that RTFS_POISON_WS already poisons keeps its own pattern."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import rtfs_oracle as O
from oracle import video_oracle as V
from oracle.video_ref64 import video_frontend64
from tests.test_hip_long_separator import VBLK, dev, host, launches, lib, model
from tests.util import frame_rel_err, l2_rel, rand, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
ERR_WORKSPACE = -2
VSD = V.make_video_state_dict(0)
_CACHE = {}


def video_model():
    import rtfs_net_amd as R
    if "video" not in _CACHE:
        m = R.FRCNNVideoModel(print_macs=False)
        m.load_state_dict({n: torch.from_numpy(np.asarray(v)) for n, v in VSD.items()})
        _CACHE["video"] = m.cuda().eval()
    return _CACHE["video"]


def lips_and_ref(B, T, seed):
    """make_video_input(B, T, seed) and its float64 embedding: computed once, shared by the tests and patterns, never written to."""
    key = ("ref", B, T, seed)
    if key not in _CACHE:
        x = V.make_video_input(B, T, seed)
        ref = video_frontend64(x, VSD)
        ref.setflags(write=False)
        _CACHE[key] = (x, ref)
    return _CACHE[key]


def vp_ref(shape, seed):
    key = ("vp",) + tuple(shape) + (seed,)
    if key not in _CACHE:
        v = rand(shape, seed)
        _CACHE[key] = (v, O.vp_block(v, VBLK))
    return _CACHE[key]


@pytest.fixture(params=[0xFF, 0x7F], ids=["nan", "big"])
def poison(request, monkeypatch):
    from rtfs_net_amd import _lib
    if _lib._POISON is None:
        monkeypatch.setattr(_lib, "_POISON", request.param)
    return _lib._POISON


def close(name, got, ref, frames=True):
    """The inference bars on the whole tensor and, for (B, 512, T) embeddings, the same 1e-4 on every frame's own scale."""
    assert got.shape == ref.shape, f"{name}: shape {got.shape} != {ref.shape}"
    e, l2 = rel_err(got, ref), l2_rel(got, ref)
    fe = frame_rel_err(got, ref) if frames else float("nan")
    print(f"[video edges] {name}: max-rel {e:.3e}  l2-rel {l2:.3e}  worst frame {fe:.3e}")
    assert np.isfinite(got).all(), f"{name}: non-finite values"
    assert e <= TOL and l2 <= TOL / 10, f"{name}: max-rel {e:.3e} l2-rel {l2:.3e}"
    if frames:
        assert fe <= TOL, f"{name}: worst frame {fe:.3e}"


# ---------------------------------------------------------------- a. the front-end at the tile edges
# (1, 1): one frame, a clip shorter than the 5-deep stem, layer 4 has 9 live pixels of 128
# (3, 2): clip boundaries inside the batch (b = n / T must not leak across clips)
# (1, 29): layer 3 = 1044 px = 9 tiles: first second round with ncb = 2, 1 live tile of 8 in it
# (2, 57): N = 114: layer 4 = 1026 px = 9 tiles: first second round with ncb = 4; layer 3 = 33 tiles = 5 rounds
# (1, 115): the same with the partial tile one frame further
# (1, 229): layer 4 = 2061 px = 17 tiles, a third round; layer 2 = 217 tiles
FRONTEND_CASES = [(1, 1, 0), (3, 2, 1), (1, 29, 2), (2, 57, 3), (1, 115, 4), (1, 229, 5)]


@pytest.mark.parametrize("B,T,seed", FRONTEND_CASES)
def test_frontend_vs_float64(B, T, seed, poison):
    x, ref = lips_and_ref(B, T, seed)
    with torch.no_grad():
        y = host(video_model()(dev(x)))
    assert y.shape == (B, 512, T)
    close(f"frontend B={B} T={T} poison {poison:#x}", y, ref)


# ---------------------------------------------------------------- b. the plain entry through the C ABI
def test_frontend_entry_point_exact_workspace(poison):
    from rtfs_net_amd import _lib
    B, T, seed = 2, 57, 3
    x, ref = lips_and_ref(B, T, seed)
    L, m = lib(), video_model()
    pk, xd = m.pack(), dev(x)
    n = L.rtfs_video_workspace_bytes(B, T)
    buf = torch.empty(n + _lib.GUARD_BYTES, dtype=torch.uint8, device="cuda").fill_(poison)  # exactly n bytes, then the guard band
    out = torch.empty(B, 512, T, device="cuda")
    out.untyped_storage().fill_(poison)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(pk.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, T, ctypes.c_void_p(buf.data_ptr()))
    rc = L.rtfs_video_frontend_f32(*args, n, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool(buf[n:].eq(poison).all()), "rtfs_video_frontend_f32 wrote past rtfs_video_workspace_bytes(B, T)"
    close(f"rtfs_video_frontend_f32 B={B} T={T} poison {poison:#x}", host(out), ref)
    # one byte short: the workspace error, and nothing launched
    out.untyped_storage().fill_(poison)
    torch.cuda.synchronize()
    n0 = L.rtfs_debug_launch_count()
    rc = L.rtfs_video_frontend_f32(*args, n - 1, st)
    torch.cuda.synchronize()
    assert rc == ERR_WORKSPACE, rc
    assert L.rtfs_debug_launch_count() == n0
    assert bool(out.view(torch.uint8).eq(poison).all())


# ---------------------------------------------------------------- c. the windows entry past 114 rows
def test_windows_entry_152_rows_vs_float64(poison):
    """Four slots x one chunk of 40 prepared frames in a single push: 38 embeddings per slot become final, 152 rows in one
    rtfs_video_frontend_windows_f32 call (layer 4 past its first round); the flush adds the two owed per slot."""
    S, F, seed = 4, 40, 6
    x, ref = lips_and_ref(S, F, seed)
    pool = video_model().open_streams(S, max_frames=F)
    ids = list(range(S))
    chunks = [dev(x[s, 0]) for s in ids]
    rows = pool._plan(ids, [F] * S, False)[2][0]
    assert 114 <= rows <= pool.max_batch_frames, rows  # one trunk call carries them all
    first, n_push = launches(lambda: pool.push(ids, chunks))
    first = [host(o) for o in first]
    last, n_flush = launches(lambda: pool.flush(ids))
    last = [host(o) for o in last]
    assert sum(o.shape[1] for o in first) == rows
    print(f"[video edges] windows entry: {rows} rows in the push tick, {n_push} launches (flush tick of {sum(o.shape[1] for o in last)} rows: {n_flush})")
    assert n_push <= n_flush, (n_push, n_flush)  # ingest + one trunk; the flush tick is ingest + one trunk + reset
    got = np.stack([np.concatenate([first[s], last[s]], axis=1) for s in ids])
    close(f"windows entry {S} x {F} frames poison {poison:#x}", got, ref)


# ---------------------------------------------------------------- d. VP block, short instance, at its length edges
# 1 .. 3: every pyramid level of length 1 or 2; 8 / 9, 16 / 17, 64 / 65 step the pyramid lengths; 112 / 113: Lg 14 -> 15;
# 120: the largest all-LDS carve-up (test_hip_long_separator's sweep starts at 121)
@pytest.mark.parametrize("tv", [1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 112, 113, 119, 120])
def test_vp_block_short(tv, poison):
    m = model()
    v, ref = vp_ref((2, 512, tv), 300 + tv)
    vd = dev(v)
    y, n = launches(lambda: m.refinement_module.video_net.blocks(vd))
    close(f"vp block Tv={tv} poison {poison:#x}", host(y), ref, frames=False)
    assert n == 1, f"Tv={tv}: {n} launches (fused VP block: 1)"


def test_vp_block_entry_point_120_batch_3(poison):
    """Three workgroups of one launch at the largest all-LDS carve-up."""
    L = lib()
    blk = model().refinement_module.video_net.get_block(0)
    v, ref = vp_ref((3, 512, 120), 920)
    x = dev(v)
    out = torch.empty_like(x)
    out.untyped_storage().fill_(poison)
    pk = blk.pack_vp()
    torch.cuda.synchronize()
    n0 = L.rtfs_debug_launch_count()
    rc = L.rtfs_vp_block_f32(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(pk.data_ptr()), ctypes.c_void_p(out.data_ptr()), 3, 120,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert L.rtfs_debug_launch_count() - n0 == 1
    close(f"rtfs_vp_block_f32 B=3 Tv=120 poison {poison:#x}", host(out), ref, frames=False)
