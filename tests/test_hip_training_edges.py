"""Boundary sweeps of the training side, the counterpart of the forward path's length / frame-count / batch sweeps: the hand-tiled GEMMs at
their K forms, M tiles and split-K chunk edges (with NaN pre-fill and guard rows), the SRU scan's 8-step look-ahead at L < 8, 8k and
8k +- 1, the training DualPathRNN over the sweep lengths where the forward bugs lived (slots of L + 7 rows, 256-position dp_ln chunks, the
fold-mode GEMM), the video-side row primitives called by name through the C ABI up to the corners include/rtfs_amd.h promises, and the
TF attention at and next to the multiples of 64 it pads T to.  References are float64 numpy or float64 torch autograd; every bound is
the one the existing test of the same kernel uses (tests/test_hip_training.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import rtfs_oracle as O
from oracle.params import make_state_dict
from tests.test_hip_parity import BLK, close, dev, host
from tests.test_hip_training import mhsa2d_training_case
from tests.util import rand, rel_err

pytestmark = pytest.mark.gpu

ERR_SHAPE, ERR_WORKSPACE = -1, -2  # include/rtfs_amd.h: RTFS_ERR_SHAPE, RTFS_ERR_WORKSPACE
LN_EPS = 1e-5  # what oracle/grad_oracle.py mhsa_1d_torch passes to F.layer_norm for norm1 / norm2
GUARD_ROWS = 256


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. GEMM edges
def _gemm_nt_case(M, N, K, acc):
    """kind 0 of rtfs_debug_gemm_f32 on a C of M + 256 rows: rows [0, M) start as NaN (accumulate 0) or random values (accumulate 1),
    the 256 guard rows behind them hold a known pattern and must come back bit-identical."""
    from rtfs_net_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(1000003 * M + 1009 * N + 2 * K + acc)
    A, B = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32)
    ref = A.astype(np.float64) @ B.astype(np.float64).T
    C0 = np.empty((M + GUARD_ROWS, N), np.float32)
    C0[:M] = rng.standard_normal((M, N)) if acc else np.nan
    C0[M:] = rng.standard_normal((GUARD_ROWS, N))
    C = dev(C0)
    a, b = dev(A), dev(B)
    _lib.check(lib.rtfs_debug_gemm_f32(0, _lib.ptr(a), _lib.ptr(b), _lib.ptr(C), M, N, K, acc, _lib.stream_of(a)), "gemm")
    got = host(C)
    close(f"gemm kind 0 {M}x{N}x{K} acc {acc}", got[:M], ref + (C0[:M] if acc else 0), tol=2e-5)
    assert np.array_equal(got[M:].view(np.uint32), C0[M:].view(np.uint32)), "rows past M were written"


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("K", [16, 48, 80, 1008, 32, 96])
def test_gemm_nt_k_forms(K, acc):
    """K % 32 == 16 is the 32x32x16 MFMA form (gemm_nt_kernel<0>, <1>: one 16-wide step up to 63 of them, the look-ahead's clamp at
    K - 16); K = 32 and 96 are the one- and three-step loops of the 16x16x32 form.  M = 257: two workgroups, the second with one row."""
    _gemm_nt_case(257, 128, K, acc)


@pytest.mark.parametrize("M,N", [(M, 64) for M in (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2305)]
                         + [(2049, 576), (2049, 192)])
def test_gemm_nt_m_edges(M, N):
    """The 64-row wave tile, the 256-row workgroup and the grid swizzle that groups row blocks by eight (M > 2048 starts the second
    group; N = 576 and 192 make the column-block count 9 and 3, neither a power of two)."""
    _gemm_nt_case(M, N, 64, 0)


@pytest.mark.parametrize("M,N,K", [(64, 64, K) for K in (1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 1279, 1281)]
                         + [(128, 192, 257), (128, 192, 1025)])
def test_gemm_tn_k_chunk_edges(M, N, K):
    """kind 1 (split K): at these sizes kchunk is 256 and a workgroup's four waves take four consecutive chunks, so K = 256 c and
    256 c +- 1 put the end of K on a chunk edge, K = 1024 / 1025 on a workgroup edge (1025: a second workgroup with one row of K and
    three empty waves), K = 1279 / 1281 on the edge of its first chunk.  C starts as random values: the kernel adds."""
    from rtfs_net_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(1000003 * M + 1009 * N + K)
    A, B = rng.standard_normal((K, M)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
    A[:, 0] *= 1e-12  # a column far below f16's range: bf16 keeps the exponent
    ref = A.astype(np.float64).T @ B.astype(np.float64)
    C0 = rng.standard_normal((M, N)).astype(np.float32)
    C0[0] = 0
    C = dev(C0)
    a, b = dev(A), dev(B)
    _lib.check(lib.rtfs_debug_gemm_f32(1, _lib.ptr(a), _lib.ptr(b), _lib.ptr(C), M, N, K, 0, _lib.stream_of(a)), "gemm")
    close(f"gemm kind 1 {M}x{N}x{K}", host(C), ref + C0, tol=2e-5)
    close("gemm tiny column", host(C)[0], ref[0], tol=2e-5)


# ------------------------------------------------------------------------------------------------ 2. SRU scan edges
@pytest.mark.parametrize("L,N", [(L, N) for L in (1, 2, 7, 8, 9, 15, 16, 17) for N in (1, 4, 5)] + [(33, 8)])
def test_sru_training_scan_edges(L, N):
    """sru.SRU forward (saved state) and backward at the scan's look-ahead edges: fewer steps than the 8 it loads ahead, exactly 8k,
    8k +- 1; one sequence, a full workgroup of four, four plus one.  Oracle and bounds of test_sru_training_forward_backward."""
    import rtfs_net_amd as R
    from oracle import grad_oracle as G
    p = O._sub(BLK, "globalatt.0")
    layers = O._sru_layers(p)
    sru = R.layers.SRU(512, 32, num_layers=4, bidirectional=True)
    sru.load_state_dict({k[len("rnn."):]: torch.from_numpy(v) for k, v in p.items() if k.startswith("rnn.")})
    sru = sru.cuda().train()
    seed = 2000 + 16 * L + N
    x = rand((L, N, 512), seed)
    dh = rand((L, N, 64), seed + 1000)
    xt = dev(x).requires_grad_(True)
    h, _ = sru(xt)
    h.backward(dev(dh))
    h_ref, dx_ref, g_ref = G.sru_grads(x, layers, dh)
    close("sru train forward", host(h), h_ref)
    close("sru dx", host(xt.grad), dx_ref, tol=2e-4)
    for i, cell in enumerate(sru.rnn_lst):
        close(f"sru layer {i} dW", host(cell.weight.grad), g_ref[i][0], tol=2e-4)
        close(f"sru layer {i} dweight_c", host(cell.weight_c.grad), g_ref[i][1], tol=2e-4)
        close(f"sru layer {i} dbias", host(cell.bias.grad), g_ref[i][2], tol=2e-4)
    with torch.no_grad():  # inference kernel and training forward agree
        close("sru eval vs train forward", host(sru(dev(x))[0]), host(h))


# ------------------------------------------------------------------------------------------------ 3. training DualPathRNN over sweep lengths
def _dp_shape(idx, Ls, B=1, other=3):
    return (B, 64, other, Ls) if idx == 0 else (B, 64, Ls, other)  # globalatt.0 sweeps the last axis (dim 4), globalatt.1 the time axis


DP_SRU = [(idx, Ls, 1, 3) for idx in (0, 1) for Ls in (8, 9, 15, 16, 17, 63, 65, 71, 121, 129, 135, 249, 256)] + [(0, 17, 2, 5), (1, 17, 2, 5)]


@pytest.mark.parametrize("idx,Ls,B,other", DP_SRU)
def test_dualpath_training_sweep_lengths(idx, Ls, B, other):
    """DualPathRNN (SRU cell) forward + backward over sweep lengths: 8 (the shortest, one window per sequence), around 16, the 65-71 and
    129-135 bands where the forward sweep's bugs lived, 249 (+ 7 pad rows = one whole 256-position dp_ln chunk) and 256 (the longest
    the backward accepts).  Three sequences of one batch entry, and ten of two (seq_base crosses a batch entry).  The backward's
    fold-mode GEMM (gemm_nt_kernel<2>) runs only here and in the other dual-path tests.  Oracle and bounds of
    test_dualpath_training_forward_backward."""
    import rtfs_net_amd as R
    from oracle import grad_oracle as G
    p = O._sub(BLK, f"globalatt.{idx}")
    dim = 4 if idx == 0 else 3
    mod = R.layers.DualPathRNN(64, 32, dim, kernel_size=8, stride=1, rnn_type="SRU", num_layers=4, bidirectional=True)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    mod = mod.cuda().train()
    shape, seed = _dp_shape(idx, Ls, B, other), 3000 + 2 * Ls + idx + 1000 * B
    x = rand(shape, seed)
    dout = rand(shape, seed + 5000)
    xt = dev(x).requires_grad_(True)
    out = mod(xt)
    out.backward(dev(dout))
    o_ref, dx_ref, g_ref = G.dualpath_grads(x, p, dim, dout)
    close("dualpath train forward", host(out), o_ref)
    close("dualpath dx", host(xt.grad), dx_ref, tol=2e-4)
    got = {k: v.grad for k, v in mod.named_parameters()}
    assert set(got) == set(g_ref)
    for k in sorted(g_ref):
        close(f"dualpath d {k}", host(got[k]).reshape(g_ref[k].shape), g_ref[k], tol=2e-4)
    if Ls <= (R.layers.FUSED_MAX_SWEEP if dim == 3 else R.layers.FUSED_MAX_BLOCK_SWEEP):  # else eval() runs the training kernels too
        with torch.no_grad():
            close("dualpath eval vs train forward", host(mod(dev(x))), host(out))


DP_CELL_LS = (8, 9, 17, 65, 129, 256)


@pytest.mark.parametrize("Ls", DP_CELL_LS)
def test_dualpath_lstm_training_sweep_lengths(Ls):
    """DualPathRNN with the LSTM cell along the time axis at the sweep-length edges; oracle (stock nn.LSTM in float64) and bounds of
    test_dualpath_lstm_training_forward_backward."""
    import json
    import rtfs_net_amd as R
    from oracle import grad_oracle as G
    from tests.util import ROOT
    spec = json.load(open(os.path.join(ROOT, "tests", "golden", "state_spec_R4_lstm.json")))
    p = O._sub(O._sub(make_state_dict(spec, 0), "refinement_module.audio_net.blocks"), "globalatt.1")
    mod = R.layers.DualPathRNN(64, 32, 3, kernel_size=8, stride=1, rnn_type="LSTM", num_layers=4, bidirectional=True)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    mod = mod.cuda().train()
    shape, seed = _dp_shape(1, Ls), 4000 + Ls
    x, dout = rand(shape, seed), rand(shape, seed + 5000)
    xt = dev(x).requires_grad_(True)
    out = mod(xt)
    out.backward(dev(dout))
    o_ref, dx_ref, g_ref = G.module_grads(lambda a, b: G.dualpath_lstm_torch(a, b, 3), x, p, dout)
    close("dualpath lstm train forward", host(out), o_ref)
    close("dualpath lstm dx", host(xt.grad), dx_ref, tol=2e-4)
    got = {k: v.grad for k, v in mod.named_parameters()}
    assert set(got) == set(g_ref)
    errs = {k: rel_err(host(got[k]).reshape(g_ref[k].shape), g_ref[k]) for k in sorted(g_ref)}
    print(f"[parity] dualpath lstm {len(g_ref)} parameter gradients: worst max-rel {max(errs.values()):.3e}")
    bad = {k: e for k, e in errs.items() if not e <= 2e-4}
    assert not bad, bad
    if Ls <= R.layers.FUSED_MAX_BLOCK_SWEEP:  # else eval() runs the training kernels too
        close("dualpath lstm eval vs train forward", host(mod.eval()(dev(x))), host(out))


@pytest.mark.parametrize("Ls", DP_CELL_LS)
def test_dualpath_gru_training_sweep_lengths(Ls):
    """DualPathRNN with the GRU cell along the time axis at the sweep-length edges; oracle (stock nn.GRU in float64) and bounds of
    test_dualpath_gru_forward_and_backward."""
    import rtfs_net_amd as R
    from oracle import grad_oracle as G
    torch.manual_seed(5000 + Ls)
    mod = R.layers.DualPathRNN(64, 32, 3, kernel_size=8, stride=1, rnn_type="GRU", num_layers=4, bidirectional=True)
    with torch.no_grad():
        mod.norm.gamma.add_(0.2 * torch.randn_like(mod.norm.gamma))
        mod.norm.beta.add_(0.2 * torch.randn_like(mod.norm.beta))
    p = {k: v.detach().numpy().copy() for k, v in mod.state_dict().items()}
    mod = mod.cuda().train()
    shape, seed = _dp_shape(1, Ls), 5000 + Ls
    x, dout = rand(shape, seed), rand(shape, seed + 5000)
    xt = dev(x).requires_grad_(True)
    out = mod(xt)
    out.backward(dev(dout))
    o_ref, dx_ref, g_ref = G.module_grads(lambda a, b: G.dualpath_lstm_torch(a, b, 3), x, p, dout)
    close("dualpath gru train forward", host(out), o_ref)
    close("dualpath gru dx", host(xt.grad), dx_ref, tol=2e-4)
    got = {k: v.grad for k, v in mod.named_parameters()}
    assert set(got) == set(g_ref)
    errs = {k: rel_err(host(got[k]).reshape(g_ref[k].shape), g_ref[k]) for k in sorted(g_ref)}
    print(f"[parity] dualpath gru {len(g_ref)} parameter gradients: worst max-rel {max(errs.values()):.3e}")
    bad = {k: e for k, e in errs.items() if not e <= 2e-4}
    assert not bad, bad
    with torch.no_grad():
        close("dualpath gru inference forward", host(mod.eval()(dev(x))), o_ref)


# ------------------------------------------------------------------------------------------------ 4. video-side row primitives (C ABI)
@pytest.mark.parametrize("N,C", [(N, C) for C in (64, 128, 512, 1024) for N in (1, 3, 4, 5)] + [(4097, 64), (4101, 128)])
def test_layernorm_rows_c_abi(N, C):
    """rtfs_layernorm_rows_f32 / _backward_f32 by name: every channel count class (1, 2, 8, 16 channels per lane), fewer rows than a
    workgroup's four waves, exactly four, four plus one, and N > 4096 where the grid (capped at 1024 workgroups of 4 rows) starts its
    grid-stride loop.  Reference: float64 F.layer_norm with the oracle's eps under autograd.  Bound 1e-5 (the masked mha_core test's) for y, dx, dgamma and dbeta,
    the sums over 4097 / 4101 rows included: a float32 numpy restatement of those sums on these
    inputs, added strictly one row after the other (the least favourable order), is 1.8e-6 from float64 for dgamma and 1.7e-6 for dbeta,
    so the bound is not widened."""
    from rtfs_net_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(7 * N + C)
    x = (rng.standard_normal((N, C)) * (1 + rng.random((N, 1))) + rng.standard_normal((N, 1))).astype(np.float32)
    gamma = (1.5 + 0.5 * rng.standard_normal(C)).astype(np.float32)  # away from 1 ...
    beta = (0.7 + 0.5 * rng.standard_normal(C)).astype(np.float32)  # ... and from 0
    dy = rng.standard_normal((N, C)).astype(np.float32)
    xr, gr, br = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, gamma, beta)]
    yr = torch.nn.functional.layer_norm(xr, (C,), gr, br, LN_EPS)
    yr.backward(torch.tensor(dy, dtype=torch.float64))
    xd, gd, bd, dyd = dev(x), dev(gamma), dev(beta), dev(dy)
    y, dx, dg, db = _nan(N, C), _nan(N, C), _nan(C), _nan(C)
    st = _lib.stream_of(xd)
    _lib.check(lib.rtfs_layernorm_rows_f32(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(y), N, C, st), "rtfs_layernorm_rows_f32")
    _lib.check(lib.rtfs_layernorm_rows_backward_f32(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(dyd), _lib.ptr(dx), _lib.ptr(dg), _lib.ptr(db), N, C, st),
               "rtfs_layernorm_rows_backward_f32")
    close(f"ln rows {N}x{C} y", host(y), yr.detach().numpy(), tol=1e-5)
    close(f"ln rows {N}x{C} dx", host(dx), xr.grad.numpy(), tol=1e-5)
    close(f"ln rows {N}x{C} dgamma", host(dg), gr.grad.numpy(), tol=1e-5)
    close(f"ln rows {N}x{C} dbeta", host(db), br.grad.numpy(), tol=1e-5)


def _linear_rows_call(lib, _lib, x, W, bias, dy, ws, ws_bytes):
    """Both entry points on NaN-filled outputs; returns (rc forward, rc backward, y, dx, dW, dbias)."""
    M, K = x.shape
    N = W.shape[0]
    y, dx, dW = _nan(M, N), _nan(M, K), _nan(N, K)
    db = _nan(N) if bias is not None else None
    st = _lib.stream_of(x)
    rc_f = lib.rtfs_linear_rows_f32(_lib.ptr(x), _lib.ptr(W), _lib.ptr(bias), _lib.ptr(y), M, N, K, st)
    rc_b = lib.rtfs_linear_rows_backward_f32(_lib.ptr(x), _lib.ptr(W), _lib.ptr(dy), _lib.ptr(dx), _lib.ptr(dW), _lib.ptr(db), M, N, K,
                                             _lib.ptr(ws), ws_bytes, st)
    return rc_f, rc_b, y, dx, dW, db


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (255, 192, 64), (257, 64, 192), (513, 128, 128)])
def test_linear_rows_c_abi(M, N, K, with_bias):
    """rtfs_linear_rows_f32 / _backward_f32 by name, with a bias and with bias = dbias = NULL, on a NaN-filled workspace of exactly
    N.K floats: y, dx, dW and dbias against float64."""
    from rtfs_net_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(M + 3 * N + 7 * K)
    x, W, dy = [rng.standard_normal(s).astype(np.float32) for s in ((M, K), (N, K), (M, N))]
    b = (0.5 + rng.standard_normal(N)).astype(np.float32) if with_bias else None
    x64, W64, dy64 = [a.astype(np.float64) for a in (x, W, dy)]
    ws = _nan(N * K)
    rc_f, rc_b, y, dx, dW, db = _linear_rows_call(lib, _lib, dev(x), dev(W), dev(b) if with_bias else None, dev(dy), ws, 4 * N * K)
    _lib.check(rc_f, "rtfs_linear_rows_f32")
    _lib.check(rc_b, "rtfs_linear_rows_backward_f32")
    close(f"linear rows {M}x{N}x{K} y", host(y), x64 @ W64.T + (b.astype(np.float64) if with_bias else 0), tol=2e-5)
    close(f"linear rows {M}x{N}x{K} dx", host(dx), dy64 @ W64, tol=2e-5)
    close(f"linear rows {M}x{N}x{K} dW", host(dW), dy64.T @ x64, tol=2e-5)
    if with_bias:
        close(f"linear rows {M}x{N}x{K} dbias", host(db), dy64.sum(0), tol=2e-5)


def test_linear_rows_refusals():
    """One workspace byte short is RTFS_ERR_WORKSPACE and N = 96 is RTFS_ERR_SHAPE, both before any launch: the launch counter stands
    still and every output keeps its NaN fill."""
    from rtfs_net_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(96)
    for (M, N, K), short, want_f, want_b in [((5, 128, 64), 1, 0, ERR_WORKSPACE), ((5, 96, 64), 0, ERR_SHAPE, ERR_SHAPE)]:
        x, W, dy, b = [dev(rng.standard_normal(s).astype(np.float32)) for s in ((M, K), (N, K), (M, N), (N,))]
        ws = _nan(N * K)
        torch.cuda.synchronize()
        n0 = lib.rtfs_debug_launch_count()
        rc_f, rc_b, y, dx, dW, db = _linear_rows_call(lib, _lib, x, W, b, dy, ws, 4 * N * K - short)
        n = lib.rtfs_debug_launch_count() - n0
        assert (rc_f, rc_b) == (want_f, want_b), (M, N, K, rc_f, rc_b)
        assert n == (1 if want_f == 0 else 0), n  # the accepted forward is one GEMM launch; the refused calls launch nothing
        for name, t in (("dx", dx), ("dW", dW), ("dbias", db), ("ws", ws)) + ((("y", y),) if want_f else ()):
            assert bool(torch.isnan(t).all()), f"{name} was written by a refused call"


def _mha_core_case(B, T, nh, hd, masked):
    from rtfs_net_amd import _lib
    lib = _lib.load()
    E = nh * hd
    rng = np.random.default_rng(1000 * T + 10 * hd + nh + (5 if masked else 0))
    qkv = rand((B, T, 3 * E), 7 + T)
    do = rand((B, T, E), 8 + T)
    mask = (rng.random((B * nh, T, T)) >= 0.3).astype(np.float32) / 0.7 if masked else None
    qr = torch.tensor(qkv, dtype=torch.float64, requires_grad=True)
    q, k_, v_ = [t.reshape(B, T, nh, hd).transpose(1, 2) for t in qr.split(E, -1)]
    a = torch.softmax(q @ k_.transpose(-1, -2) / np.sqrt(float(hd)), -1)
    if masked:
        a = a * torch.tensor(mask, dtype=torch.float64).reshape(B, nh, T, T)
    o_ref = (a @ v_).transpose(1, 2).reshape(B, T, E)
    o_ref.backward(torch.tensor(do, dtype=torch.float64))
    qd, dod, md = dev(qkv), dev(do), (dev(mask) if masked else None)
    o, dqkv = _nan(B, T, E), _nan(B, T, 3 * E)
    st = _lib.stream_of(qd)
    tag = f"mha core B{B} T{T} heads {nh} x {hd}{' masked' if masked else ''}"
    _lib.check(lib.rtfs_mha_core_f32(_lib.ptr(qd), _lib.ptr(md), _lib.ptr(o), B, T, nh, hd, st), "rtfs_mha_core_f32 " + tag)
    _lib.check(lib.rtfs_mha_core_backward_f32(_lib.ptr(qd), _lib.ptr(md), _lib.ptr(dod), _lib.ptr(dqkv), B, T, nh, hd, st),
               "rtfs_mha_core_backward_f32 " + tag)
    close(tag + " forward", host(o), o_ref.detach().numpy(), tol=1e-5)
    close(tag + " d qkv", host(dqkv), qr.grad.numpy(), tol=1e-5)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,T,nh,hd", [(1, 1, 1, 8), (2, 2, 3, 1), (1, 63, 2, 16), (1, 64, 2, 16), (2, 65, 3, 5), (1, 255, 1, 8), (1, 256, 2, 8),
                                       (1, 237, 1, 16)])
def test_mha_core_c_abi(B, T, nh, hd, masked):
    """rtfs_mha_core_f32 / _backward_f32 by name over the promised range: one position, head_dim 1, T at and next to the wave size,
    T = 255 / 256 (every thread of the workgroup owns a row), head_dim 16, and (237, 16): 63,516 bytes of dynamic LDS, the most below
    64 KiB.  Without and with a dropout keep-mask (p = 0.3); the float64 formula and bound of test_video_mhsa_training_forward_backward."""
    _mha_core_case(B, T, nh, hd, masked)


def test_mha_core_refusals():
    """T = 257 and head_dim = 17 are outside the contract: RTFS_ERR_SHAPE from both entry points, nothing launched, nothing written."""
    from rtfs_net_amd import _lib
    lib = _lib.load()
    for T, hd in [(257, 8), (8, 17)]:
        qd, dod = dev(rand((1, T, 3 * hd), 1)), dev(rand((1, T, hd), 2))
        o, dqkv = _nan(1, T, hd), _nan(1, T, 3 * hd)
        st = _lib.stream_of(qd)
        torch.cuda.synchronize()
        n0 = lib.rtfs_debug_launch_count()
        assert lib.rtfs_mha_core_f32(_lib.ptr(qd), None, _lib.ptr(o), 1, T, 1, hd, st) == ERR_SHAPE
        assert lib.rtfs_mha_core_backward_f32(_lib.ptr(qd), None, _lib.ptr(dod), _lib.ptr(dqkv), 1, T, 1, hd, st) == ERR_SHAPE
        assert lib.rtfs_debug_launch_count() == n0
        assert bool(torch.isnan(o).all()) and bool(torch.isnan(dqkv).all())


# ------------------------------------------------------------------------------------------------ 5. TF attention at padded-T boundaries
@pytest.mark.parametrize("T", [63, 64, 65, 128, 129, 192, 193])
def test_mhsa2d_training_padded_t_edges(T):
    """MultiHeadSelfAttention2D inside a training step with T at and next to the multiples of 64 the batched GEMMs pad it to (Tp = T: no
    padding; Tp - T = 1 and 63: the least and the most); body, oracle and bounds of test_mhsa2d_training_forward_backward."""
    mhsa2d_training_case((1, 64, T, 64), 400 + T)


# the one launch nobody had made before this file: kept last, so that whatever it does cannot reach the cases above
@pytest.mark.parametrize("masked", [False, True])
def test_mha_core_largest_lds_corner(masked):
    """T = 256 with head_dim = 16, the corner of the header's contract: (4.256.16 + 3.256).4 = 68,608 bytes of dynamic LDS, above the
    64 KiB a kernel may ask for without the max-dynamic-LDS attribute."""
    _mha_core_case(1, 256, 1, 16, masked)
