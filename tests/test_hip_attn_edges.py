"""Boundary sweep of the inference attention family (csrc/k_attn.hip): the three launchers, one at a time, through rtfs_debug_attn_f32,
against tests/attn_reference.py, every element compared.

Routes.  Every case states the record it expects - family, channel-last form, frames per workgroup, grid, LDS bytes, (b, head) pairs - from
the documented rule, written out below, and asserts what the launcher hands back; a refusal must leave the record empty, launch nothing
and write nothing.  The frames-per-workgroup values seen across the file must be {1, 2, 3, 4, 5, 6, 8}.

Row kernels (ops 0 and 2).  (T, B) such that every rpw occurs with T % rpw in {0, 1, rpw - 1}, with T = rpw and with T < rpw; B is the
smallest batch that reaches the rpw threshold.  Frames are independent draws, the PReLU slopes of the twelve modules all differ, gamma and
beta are random per (channel, f).  The channel-last form must reproduce the channel-major form bit for bit.

Core (op 1), T over the key-tile edges x B in {1, 2, 3} (B = 3: 12 pairs padded to 16), three tiers.
* Selection: K = +-1, Q = 16 K[pi], integer V: scores are exact integers, the chosen key's 256 at least 110 above the runner-up, so the
  float32 softmax is exactly one-hot and the output must EQUAL V[pi]: no tolerance.
* Uniform: Q = 0, every row is the mean of the T real V rows: the case that fails when a padded key gets weight.
* Float: Q, K, V as the QKV stage makes them (unit scale times gamma near 8, plus beta), scores scaled to a standard deviation near 2.

Float bars: per stage ten times the worst value of the same measure for the CPU emulation (attn_reference.F16X3) on the same inputs,
never above 1e-5.

Buffers: every output is followed by a guard band of 8 rows of the widest row any launcher writes (8 x 1024 floats), which must keep its
bits; outputs start as NaN (or the poison of a poisoned run), unused pointers are null, the bands behind inputs are NaN.  The output
layouts have no pitch: the element behind the last row of a channel plane (a (b, head) slice) is the first of the next plane, which another
workgroup writes - a store past a plane's end is therefore seen by the every-element comparison of the next plane or, behind the last
plane, by the band.  No case is meant to fault: every shape satisfies its launcher's preconditions or is one the launcher refuses."""
import ctypes

import numpy as np
import pytest
import torch

from tests import attn_reference as A
from tests.test_hip_parity import close, host

pytestmark = pytest.mark.gpu

ERR_SHAPE, ERR_ARG = -1, -4
QKV, CORE, PROJ = 1, 2, 3        # route families (include/rtfs_amd.h)
GUARD = 8 * 1024
SEEN_RPW = set()                 # frames per workgroup of every row route asserted in this file
WORST = {}                       # stage -> (emulation worst, GPU worst) over the file
FLOAT = {}                       # section -> [(case, tensor, GPU error, emulation error)]
CORE_TS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 288, 289, 384, 385, 415, 416, 417, 511, 512]


def cdiv(a, b):
    return -(-a // b)


def rcan_rows(T, B):
    """Frames per workgroup of the row kernels, the documented rule (k_attn.hip): 8 once the launch has 3500 frames, below that one per 512
    frames, at least 1."""
    n = T * B
    if n >= 3500:
        return 8
    return max(1, min(8, n // 512))


def row_route(family, cl, T, B):
    rpw = rcan_rows(T, B)
    return (family, cl, rpw, cdiv(T, rpw), B, 0, 0)


def core_route(T, B):
    nkt = cdiv(T, 32)
    return (CORE, 0, 0, cdiv(4 * B, 8) * 8 * nkt, 1, 32 * (32 * nkt + 4) * 4, 4 * B)


def _L():
    from rtfs_net_amd import _lib as L
    return L.load(), L


def vscale():
    """The power of two V is stored times between the QKV rows and the core: op 0 writes v so, op 1 reads it so (include/rtfs_amd.h)."""
    s = _L()[0].rtfs_debug_attn_vscale()
    assert s == A.VSC
    return np.float32(s)


def dv(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


class Buf:
    """A device tensor of `shape` behind which a guard band lies (tests/test_hip_pw_edges.py Buf without a row pitch).  Inputs (`init`) are
    followed by NaN; outputs are NaN, or what _lib.empty gave under a poisoned run, and their band must come back untouched."""

    def __init__(self, shape, init=None):
        _, L = _L()
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.t = L.empty(self.n + GUARD, device="cuda")
        if init is not None:
            self.t[:self.n] = dv(init).reshape(-1)
            self.t[self.n:] = float("nan")
        else:
            if L._POISON is None:
                self.t[:self.n] = float("nan")
            self.t[self.n:] = torch.arange(GUARD, dtype=torch.float32, device="cuda") + 0.5
        self.before = host(self.t[self.n:]).copy() if init is None else None
        self.whole = None

    def ptr(self):
        return self.t.data_ptr()

    def take(self, name):
        h = host(self.t)
        assert np.array_equal(h[self.n:].view(np.uint32), self.before.view(np.uint32)), f"{name}: written past its end"
        return h[:self.n].reshape(self.shape)

    def snapshot(self):
        self.whole = host(self.t).copy()
        return self

    def untouched(self, name):
        assert np.array_equal(host(self.t).view(np.uint32), self.whole.view(np.uint32)), f"{name}: written by a refused call"


NAMES = "x res wt bias slope gamma beta q k v out".split()


def call(op, B, T, cl=0, scale=0.0, n_ints=3, **ptrs):
    """-> (status, launches, [route tuples]).  ptrs: name -> Buf, device tensor or None."""
    assert set(ptrs) <= set(NAMES), set(ptrs) - set(NAMES)
    p = []
    for n in NAMES:
        v = ptrs.get(n)
        p.append(None if v is None else v.ptr() if isinstance(v, Buf) else v.data_ptr())
    lib, _ = _L()
    ints = [B, T, cl]
    Pp = (ctypes.c_void_p * len(p))(*p)
    I = (ctypes.c_int * len(ints))(*ints)
    Dd = (ctypes.c_double * 1)(scale)
    Rt = (ctypes.c_int * 8)(*([-7] * 8))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n0 = lib.rtfs_debug_launch_count()
    rc = lib.rtfs_debug_attn_f32(op, Pp, len(p), I, n_ints, Dd, 1, Rt, 8, st)
    torch.cuda.synchronize()
    launches = lib.rtfs_debug_launch_count() - n0
    return rc, launches, [tuple(Rt[1 + 7 * i:8 + 7 * i]) for i in range(Rt[0])]


def ok(name, res, route):
    rc, n, got = res
    assert rc == 0, f"{name}: status {rc}"
    assert got == [route], f"{name}: route {got} != {[route]}"
    assert n == 1, f"{name}: {n} launches"
    if route[0] != CORE:
        SEEN_RPW.add(got[0][2])


def refused(name, res, status, *bufs):
    rc, n, got = res
    assert rc == status and n == 0 and got == [], f"{name}: status {rc} (want {status}), {n} launches, route {got}"
    for b in bufs:
        b.untouched(name)


def floaty(sec, name, tensor, got, ref, den, emu):
    assert got.shape == tuple(ref.shape), f"{name} {tensor}: shape {got.shape} != {tuple(ref.shape)}"
    assert np.isfinite(got).all(), f"{name} {tensor}: non-finite output"
    FLOAT.setdefault(sec, []).append((name, tensor, A.err(got, ref, den), A.err(emu, ref, den)))


def finish(sec, stage):
    rows = FLOAT.pop(sec)
    emu = max(r[3] for r in rows)
    bar = min(10 * emu, 1e-5)
    worst = max(rows, key=lambda r: r[2])
    print(f"[attn] {sec}: {len(rows)} float tensors, f16x3 emulation worst {emu:.3e}, bar {bar:.3e}, worst GPU {worst[2]:.3e} ({worst[0]} {worst[1]})")
    w = WORST.get(stage, (0.0, 0.0))
    WORST[stage] = (max(w[0], emu), max(w[1], worst[2]))
    assert emu > 0
    bad = [r for r in rows if not r[2] <= bar]
    assert not bad, f"{sec}: {len(bad)} of {len(rows)} tensors above the bar {bar:.3e}, worst {worst[0]} {worst[1]}: {worst[2]:.3e}"


# ------------------------------------------------------------------------------------------------ routes
def test_rpw_7_is_unreachable():
    """T * B over 3072 .. 4096, one frame per sample: the launcher's own record goes 6, 6, ..., 8 at 3500 - and the documented rule gives
    7 nowhere at all."""
    assert {rcan_rows(1, n) for n in range(1, 20000)} == {1, 2, 3, 4, 5, 6, 8}
    rng = np.random.default_rng(1)
    p = A.row_params(rng, 96)
    k = dict(x=dv(A.row_input(rng, 4096, 1)), wt=dv(p["w"].T), bias=dv(p["b"]), slope=dv(p["slope"]), gamma=dv(p["gamma"]), beta=dv(p["beta"]),
             q=Buf((4096, 4, 1, 256)), k=Buf((4096, 4, 1, 256)), v=Buf((4096, 4, 1, 1024)))
    seen = set()
    for n in range(3072, 4097):
        rc, launches, got = call(0, n, 1, **k)
        assert rc == 0 and launches == 1 and got == [row_route(QKV, 0, 1, n)], (n, rc, got)
        seen.add(got[0][2])
    assert seen == {6, 8}
    for name in "qkv":
        k[name].take(name)


# ------------------------------------------------------------------------------------------------ row kernels
def row_shapes(rpw):
    """(T, B): T % rpw in {0, 1, rpw - 1}; at rpw 2, 5 and 8 also T = rpw and T < rpw (one workgroup per sample, its tail longer than
    its work); B the smallest batch whose T * B reaches the threshold of this rpw."""
    if rpw == 1:
        return [(1, 1), (5, 2), (33, 3), (125, 8)]
    lo = 3500 if rpw == 8 else 512 * rpw
    ts = sorted({4 * rpw, 4 * rpw + 1, 5 * rpw - 1} | ({rpw, 3 if rpw == 8 else rpw - 1} if rpw in (2, 5, 8) else set()))
    out = [(T, cdiv(lo, T)) for T in ts]
    assert all(rcan_rows(T, B) == rpw and (B == 1 or rcan_rows(T, B - 1) < rpw) for T, B in out)
    return out


def cl_of(x):
    """(B,64,T,64) channel-major -> (B,T,64 f,64 c) channel-last"""
    return np.ascontiguousarray(x.transpose(0, 2, 3, 1))


def row_case(sec, op, T, B):
    name = f"{sec} T{T} B{B}"
    rng = np.random.default_rng([op, T, B])
    p = A.row_params(rng, 96 if op == 0 else 64)
    x = A.row_input(rng, B, T)
    k = dict(wt=dv(p["w"].T), bias=dv(p["b"]), slope=dv(p["slope"]), gamma=dv(p["gamma"]), beta=dv(p["beta"]))
    if op == 0:
        refs, dens = A.qkv(A.EXACT, x, **p)
        emus, _ = A.qkv(A.F16X3, x, **p)
        tensors, shapes = ("q", "k", "v"), ((B, 4, T, 256), (B, 4, T, 256), (B, 4, T, 1024))
    else:
        res = rng.standard_normal((B, 64, T, 64)).astype(np.float32)
        refs, dens = A.proj(A.EXACT, x, res, **p)
        emus, _ = A.proj(A.F16X3, x, res, **p)
        tensors, shapes = ("out",), ((B, 64, T, 64),)
    got = {}
    for cl in (0, 1):
        outs = [Buf(s) for s in shapes]
        if op == 0:
            r = call(0, B, T, cl, x=Buf(x.shape, cl_of(x) if cl else x), q=outs[0], k=outs[1], v=outs[2], **k)
        else:
            r = call(2, B, T, cl, x=Buf(x.shape, x), res=Buf(res.shape, cl_of(res) if cl else res), out=outs[0], **k)
        ok(f"{name} cl{cl}", r, row_route(QKV if op == 0 else PROJ, cl, T, B))
        got[cl] = [o.take(f"{name} cl{cl} {tn}") for o, tn in zip(outs, tensors)]
        if op == 0:
            got[cl][2] = got[cl][2] / vscale()  # a power of two: exact
    for i, tn in enumerate(tensors):
        if op == 0:  # per head: a (b, head) slice of its own layout, one LayerNorm group per frame
            for h in range(4):
                floaty(sec, name, f"{tn} head {h}", got[0][i][:, h], refs[i][:, h], dens[i][:, h], emus[i][:, h])
        else:
            floaty(sec, name, tn, got[0][i], refs[i], dens[i], emus[i])
        # same fragments, same arithmetic order, only the load path differs
        assert np.array_equal(got[0][i].view(np.uint32), got[1][i].view(np.uint32)), f"{name} {tn}: channel-last differs from channel-major"


@pytest.mark.parametrize("rpw", [1, 2, 3, 4, 5, 6, 8])
def test_row_can_qkv(rpw):
    """launch_row_can_qkv -> row_can_kernel<96>, both forms: the nrows tail, the prefetch across frames, Ys reused from frame to frame, the
    slope of every module, Q / K / V head-major."""
    sec = f"qkv rpw{rpw}"
    for T, B in row_shapes(rpw):
        row_case(sec, 0, T, B)
    finish(sec, "qkv rows")


@pytest.mark.parametrize("rpw", [1, 2, 3, 4, 5, 6, 8])
def test_row_can_proj(rpw):
    """launch_row_can_proj -> row_can_kernel<64>, both forms: one LayerNorm group over (64, F) through `red`, the residual channel-major and
    through Rs."""
    sec = f"proj rpw{rpw}"
    for T, B in row_shapes(rpw):
        row_case(sec, 2, T, B)
    finish(sec, "projection rows")


# ------------------------------------------------------------------------------------------------ core
def chan(z, B, T):
    """(B,4,T,1024) -> (B,64,T,64), channel = head * 16 + c"""
    return np.ascontiguousarray(z.reshape(B, 4, T, 16, 64).transpose(0, 1, 3, 2, 4).reshape(B, 64, T, 64))


def core_run(name, q, k, v, B, T, scale=0.0):
    o = Buf((B, 64, T, 64))
    ok(name, call(1, B, T, scale=scale, q=Buf(q.shape, q), k=Buf(k.shape, k), v=Buf(v.shape, v * vscale()), out=o), core_route(T, B))
    return o.take(name)


@pytest.mark.parametrize("B", [1, 2, 3])
def test_core_selection_exact(B):
    """No tolerance: query row, key tile, wave ownership of key tiles, column interleave and the (b, head) <-> slot mapping."""
    for T in CORE_TS:
        rng = np.random.default_rng([10, B, T])
        k = rng.choice([-1.0, 1.0], (B, 4, T, 256)).astype(np.float32)
        pi = np.stack([rng.permutation(T) for _ in range(4 * B)]).reshape(B, 4, T)
        q = 16 * np.take_along_axis(k, pi[..., None], 2)
        v = rng.integers(-8, 9, (B, 4, T, 1024)).astype(np.float32)
        if T > 1:
            s = np.sort(np.matmul(q.astype(np.float64), k.astype(np.float64).transpose(0, 1, 3, 2)) / 16, -1)
            assert (s[..., -1] == 256).all() and (s[..., -1] - s[..., -2]).min() >= 110, f"T{T} B{B}: the softmax is not one-hot in float32"
        want = chan(np.take_along_axis(v, pi[..., None], 2), B, T)
        got = core_run(f"core selection T{T} B{B}", q, k, v, B, T)
        if not np.array_equal(got, want):
            i = tuple(int(j) for j in np.argwhere(~(got == want))[0])
            raise AssertionError(f"core selection T{T} B{B}: {int((~(got == want)).sum())} of {got.size} elements differ, first at (b, channel, t, f) = {i}: "
                                 f"got {got[i]!r}, want {want[i]!r}")


def uniform_cases(sec, B, Ts, stage="core"):
    for T in Ts:
        rng = np.random.default_rng([11, B, T])
        _, k, v = A.core_inputs(rng, B, T)
        q = np.zeros_like(k)
        (ref,), (den,) = A.core(A.EXACT, q, k, v)
        assert np.allclose(ref.numpy(), chan(np.broadcast_to(v.astype(np.float64).mean(2, keepdims=True), v.shape), B, T), rtol=1e-12, atol=1e-12)
        (emu,), _ = A.core(A.F16X3, q, k, v)
        floaty(sec, f"T{T} B{B}", "o", core_run(f"{sec} T{T}", q, k, v, B, T), ref, den, emu)
    finish(sec, stage)


def float_cases(sec, B, Ts, stage="core"):
    for T in Ts:
        rng = np.random.default_rng([12, B, T])
        q, k, v = A.core_inputs(rng, B, T)
        (ref,), (den,) = A.core(A.EXACT, q, k, v, A.CORE_SCALE)
        (emu,), _ = A.core(A.F16X3, q, k, v, A.CORE_SCALE)
        floaty(sec, f"T{T} B{B}", "o", core_run(f"{sec} T{T}", q, k, v, B, T, A.CORE_SCALE), ref, den, emu)
    finish(sec, stage)


@pytest.mark.parametrize("B", [1, 2, 3])
def test_core_uniform(B):
    """Q = 0: every output row is the mean of the T real V rows; the clamped copies of row T - 1 under the padded keys must get no weight."""
    uniform_cases(f"core uniform B{B}", B, CORE_TS[1:])


@pytest.mark.parametrize("B", [1, 2, 3])
def test_core_float(B):
    """Random Q, K, V; the query rows q >= T of the last tile must not be stored (see the module docstring: the next plane, or the band)."""
    float_cases(f"core float B{B}", B, CORE_TS[1:])


@pytest.mark.parametrize("B", [1, 2, 3])
def test_core_single_key_uniform(B):
    """T = 1, the one key with weight 1: the output is V[0] as the f16 split holds it, and no sum stands behind a small element.  With V
    split unscaled this missed the bar (GPU 1.5e-5 at B = 1: the low part of an element below 2^-3 is an f16 subnormal, an absolute floor
    of 2^-25); V is stored times 64 since (ATT_VSC): 1.2e-7."""
    uniform_cases(f"core single key uniform B{B}", B, CORE_TS[:1], "core, single key")


@pytest.mark.parametrize("B", [1, 2, 3])
def test_core_single_key_float(B):
    """T = 1 with random Q: as test_core_single_key_uniform (4.2e-5 at B = 1 before V was scaled, 3e-9 since)."""
    float_cases(f"core single key float B{B}", B, CORE_TS[:1], "core, single key")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    """Status as documented, nothing launched, the route record empty, every buffer bit-identical."""
    rng = np.random.default_rng(13)
    B, T = 2, 5
    q, k, v = A.core_inputs(rng, B, T)
    cb = dict(q=Buf(q.shape, q).snapshot(), k=Buf(k.shape, k).snapshot(), v=Buf(v.shape, v).snapshot(), out=Buf((B, 64, T, 64)).snapshot())
    p = A.row_params(rng, 96)
    x = A.row_input(rng, B, T)
    rb = dict(x=Buf(x.shape, x).snapshot(), q=Buf(q.shape).snapshot(), k=Buf(k.shape).snapshot(), v=Buf(v.shape).snapshot())
    rk = dict(wt=dv(p["w"].T), bias=dv(p["b"]), slope=dv(p["slope"]), gamma=dv(p["gamma"]), beta=dv(p["beta"]))
    refused("core T 513", call(1, B, 513, **cb), ERR_SHAPE, *cb.values())
    refused("core T 0", call(1, B, 0, **cb), ERR_ARG, *cb.values())
    refused("core B 0", call(1, 0, T, **cb), ERR_ARG, *cb.values())
    refused("qkv B 0", call(0, 0, T, **rb, **rk), ERR_ARG, *rb.values())
    refused("qkv T 0", call(0, B, 0, **rb, **rk), ERR_ARG, *rb.values())
    refused("short ints", call(0, B, T, n_ints=2, **rb, **rk), ERR_ARG, *rb.values())
    refused("unknown op 3", call(3, B, T, **rb, **rk), ERR_ARG, *rb.values())
    refused("unknown op -1", call(-1, B, T, **cb), ERR_ARG, *cb.values())
    refused("qkv without v", call(0, B, T, **{n: b for n, b in rb.items() if n != "v"}, **rk), ERR_ARG, *rb.values())
    refused("proj without its residual", call(2, B, T, x=rb["x"], out=cb["out"], **rk), ERR_ARG, rb["x"], cb["out"])
    # and the record of a good call does not survive into a refusal
    ok("core after the refusals", call(1, B, T, **cb), core_route(T, B))
    refused("core T 513 after a good call", call(1, B, 513, **cb), ERR_SHAPE)


# ------------------------------------------------------------------------------------------------ composite
@pytest.mark.parametrize("T,B", [(125, 9), (33, 94), (33, 107)])
def test_public_entry_with_several_frames_per_workgroup(T, B):
    """rtfs_tf_attention_f32 at module level with rpw = 2 (125 % 2 = 1), 6 (33 % 6 = 3) and 8 (33 x 107 = 3531 frames are past the 3500
    threshold; 33 % 8 = 1), against the float64 restatement on the oracle's own parameters at the module bars."""
    from oracle import rtfs_oracle as O
    from oracle.params import make_state_dict
    from tests.util import rand, spec_R4
    assert rcan_rows(T, B) == {(125, 9): 2, (33, 94): 6, (33, 107): 8}[(T, B)] and T % rcan_rows(T, B) != 0
    att = O._sub(O._sub(make_state_dict(spec_R4(), 0), "refinement_module.audio_net.blocks"), "globalatt.2")
    P = A.params_of(att)
    def piece(a):  # every piece of a pack starts on a multiple of 64 floats (include/rtfs_amd.h)
        a = np.asarray(a, np.float32).reshape(-1)
        return np.concatenate([a, np.zeros(-a.size % 64, np.float32)])
    pack = dv(np.concatenate([piece(a) for a in (
        P["qkv_w"].T, P["qkv_b"], P["qkv_slope"], P["qkv_gamma"], P["qkv_beta"], P["proj_w"].T, P["proj_b"], P["proj_slope"], P["proj_gamma"],
        P["proj_beta"])]))
    lib, L = _L()
    assert pack.numel() == lib.rtfs_pack_floats(L.PACK_ATTENTION)
    x = rand((B, 64, T, 64), 80 + T)
    xd = dv(x)
    out = L.empty(B, 64, T, 64, device="cuda")
    ws = L.workspace(lib.rtfs_tf_attention_workspace_bytes(B, T), xd.device)
    L.check(lib.rtfs_tf_attention_f32(L.ptr(xd), L.ptr(pack), L.ptr(out), B, T, L.ptr(ws), ws.numel(), L.stream_of(xd)), "rtfs_tf_attention_f32")
    close(f"rtfs_tf_attention_f32 T={T} B={B}", host(out), A.mhsa(A.EXACT, x, P).numpy())


# ------------------------------------------------------------------------------------------------ coverage of the file itself
def test_every_rpw_was_seen():
    """Over the routes asserted above (the module-level record): a sweep that reached rpw = 6 only on paper would not fill it."""
    assert SEEN_RPW == {1, 2, 3, 4, 5, 6, 8}, SEEN_RPW
    for stage, (emu, gpu) in sorted(WORST.items()):
        bar = min(10 * emu, 1e-5)
        note = "  (within 2x of the bar: the emulation is not modelling the kernel)" if gpu > bar / 2 else \
            "  (below a tenth of the emulation: the emulation is not modelling the kernel)" if gpu < emu / 10 else ""
        print(f"[attn] {stage}: f16x3 emulation {emu:.3e}, bar {bar:.3e}, GPU worst {gpu:.3e}{note}")
    assert set(WORST) == {"qkv rows", "projection rows", "core", "core, single key"}
