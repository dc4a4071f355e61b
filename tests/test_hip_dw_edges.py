"""Boundary sweeps of csrc/k_dw.hip, the inference depthwise family: every launcher, one at a time, through rtfs_debug_dw_f32, against
tests/dw_reference.py (float64, or int64 for the exact forms), every element compared.

Routes.  Every case states the route it is meant to take - kernel family, NCONV, IN_AFFINE, MODE, VAR, effective band height and logical
grid - and asserts the record the launcher hands back: a shape that silently falls to the one-column kernel must not pass for coverage of
the packed one.  Which kernel a row of the table takes is written in the table; the band height and grid are computed by the mirror of
band_rows() below.

Two comparisons.
* Exact: forms without a fold and without a sigmoid (plain writes with 1 / 2 / 3 / 4 convs, MODE 1 statistics, the row write, jobs 0 and 1
  of the three-job launch, the one-column forms) run on x, w in {-2..2}, bias in {-1, 0, 1}: every output is an integer of magnitude <= 65
  and every sum stays far below 2^24, so float32 is exact in any order and outputs and (sum, sumsq) must EQUAL the int64 reference.
* Float: everything with a fold, a sigmoid or a pool mean: max|got - ref| / max|ref| per tensor against float64.  The bar is not a
  constant: every float case also runs the same formula in float32 torch on the CPU, and a section's bar is ten times the worst error of
  that run against float64 over the section's cases (the kernels add hardware exp2 / rcp, an f32 rsqrt in the fold, FMA contraction and
  another summation order).  The section asserts at its end, and asserts that its bar stays below the project's 1e-4.
  Statistics: sumsq at rtol 1e-5 (the bar of test_encoder_stats_and_ragged_length), sum at 1e-5 of sum|y|.

Buffers: outputs come from _lib.empty (the poisoned runs reach them; NaN-filled otherwise) and are followed by a guard region that must
come back untouched; where cs > H W the guard starts at B C cs and nothing is asserted about the padding inside a channel's allocation.
Input padding is NaN: a load from it would show.  Statistics are zeroed by the caller, as block_body does.

No case is meant to fault: every shape satisfies its launcher's preconditions or is one the launcher refuses before launching."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import dw_reference as D
from tests.nearest_cases import departs
from tests.test_hip_parity import host
from tests.util import rel_err

pytestmark = pytest.mark.gpu

ERR_SHAPE, ERR_ARG = -1, -4
GUARD = 1024          # floats (doubles for statistics) behind every output
S1, P1, G3, S2X, S2POOL, S2STATS, GFORM, GCOMBINE = 1, 2, 3, 4, 5, 6, 7, 8  # route families (include/rtfs_amd.h)
ADD, SHARE, COMB, ROW, NOHALO = 1, 2, 4, 8, 16                             # VAR bits
FLOAT = {}  # section -> list of (case, tensor, gpu error, float32-restatement error)
COUNT = {}  # section -> cases run


def cdiv(a, b):
    return -(-a // b)


def band_rows(th, rows, gx, B, target):
    """Mirror of band_rows() in k_dw.hip: the requested band height holds from 512 workgroups on; below, bands shrink to multiples of 8."""
    if gx * cdiv(rows, th) * B >= 512:
        return th
    t = (cdiv(rows, cdiv(target, gx * B)) + 7) // 8 * 8
    return 8 if t < 8 else min(t, th)


def gx_packed(C, W, var=0):
    return C // 4 if var & ROW else cdiv(cdiv(C * ((W + 1) // 2), 64 if var & NOHALO else 62), 4)


def packed(nconv, aff, mode, var, B, C, H, W, TH):
    gx = gx_packed(C, W, var)
    th = band_rows(TH, H, gx, B, 768 if mode == 2 else 320)
    return (P1, nconv, int(aff), mode, var, th, gx, cdiv(H, th))


def onecol(nconv, aff, mode, C, H, W, TH):
    return (S1, nconv, int(aff), mode, 0, TH, cdiv(C * W, 256), cdiv(H, TH))


def pitch(n):
    return (n + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------ buffers and the call
def _L():
    from rtfs_net_amd import _lib as L
    return L.load(), L


def _out(n):
    """Output of n floats from _lib.empty (poisoned runs) or NaN, followed by the guard pattern."""
    _, L = _L()
    t = L.empty(n + GUARD, device="cuda")
    if L._POISON is None:
        t[:n] = float("nan")
    t[n:] = torch.arange(GUARD, dtype=torch.float32, device="cuda") + 0.5
    return t


def _take(t, n, name):
    h = host(t)
    want = np.arange(GUARD, dtype=np.float32) + 0.5
    assert np.array_equal(h[n:n + GUARD].view(np.uint32), want.view(np.uint32)), f"{name}: written past its end"
    return h[:n]


def _untouched(t, n, name):
    """After a refusal: nothing written (the NaN / poison fill is still there) and the guard is whole."""
    h = _take(t, n, name)
    _, L = _L()
    if L._POISON is None:
        assert np.isnan(h).all(), f"{name}: written by a refused call"
    else:
        assert (h.view(np.uint8) == L._POISON).all(), f"{name}: written by a refused call"


def _stats_buf(B):
    t = torch.zeros(2 * B + GUARD, dtype=torch.float64, device="cuda")
    t[2 * B:] = torch.arange(GUARD, dtype=torch.float64, device="cuda") + 0.5
    return t


def _take_stats(t, B, name):
    h = host(t)
    assert np.array_equal(h[2 * B:], np.arange(GUARD, dtype=np.float64) + 0.5), f"{name}: statistics written past their end"
    return h[:2 * B].reshape(B, 2)


def dv(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def strided(x4, cs):
    """(B, C, H, W) -> device (B, C, cs) with NaN in the padding behind every channel plane."""
    B, C, H, W = x4.shape
    buf = np.full((B, C, cs), np.nan, np.float32)
    buf[:, :, :H * W] = x4.reshape(B, C, H * W)
    return dv(buf)


def unstrided(flat, B, C, H, W, cs):
    return flat.reshape(B, C, cs)[:, :, :H * W].reshape(B, C, H, W)


def desc(**k):
    """One conv description of rtfs_debug_dw_f32: (35 pointers, 14 ints, 4 doubles).  Tensor arguments are device tensors or None."""
    p = [None] * 35
    def put(i, t):
        if t is not None:
            p[i] = t if isinstance(t, int) else t.data_ptr()
    put(0, k.get("x"))
    for i, n in enumerate(("in_stats", "in_gamma", "in_beta")):
        put(1 + i, k.get(n))
    present = 0
    w, bias, out, so = (list(k.get(n) or []) + [None] * 4 for n in ("w", "bias", "out", "stats_out"))
    for i in range(4):
        put(4 + i, w[i])
        if bias[i] is not None:
            put(8 + i, bias[i])
            present |= 1 << i
        put(12 + i, out[i])
        put(16 + i, so[i])
    for i, n in enumerate(("loc_stats", "loc_gamma", "loc_beta", "gate", "gate_stats", "gate_gamma", "gate_beta", "emb", "emb_stats",
                           "emb_gamma", "emb_beta", "addend", "add_stats", "add_gamma", "add_beta")):
        put(20 + i, k.get(n))
    if k.get("addend") is not None:
        present |= 16
    ints = [k["B"], k["C"], k["H"], k["W"], k.get("Hg", 0), k.get("Wg", 0), k.get("TH", 8), k.get("cs", 0), k.get("rev", 0),
            k.get("nconv", 1), int(k.get("in_affine", False)), k.get("mode", 0), int(k.get("in_combine", False)), present]
    dbls = [k.get("in_inv", 0.0), k.get("loc_inv", 0.0), k.get("g_inv", 0.0), k.get("add_inv", 0.0)]
    return p, ints, dbls


def call(op, *descs, flat=None):
    """-> (status, launches, [route job tuples]).  descs: desc() results, or flat = (ptrs, ints, dbls) for ops 4 and 5."""
    lib, L = _L()
    if flat is None:
        ptrs, ints, dbls = [sum((d[i] for d in descs), []) for i in range(3)]
    else:
        ptrs, ints, dbls = flat
    P = (ctypes.c_void_p * len(ptrs))(*ptrs)
    I = (ctypes.c_int * len(ints))(*ints)
    Dd = (ctypes.c_double * len(dbls))(*dbls)
    R = (ctypes.c_int * 33)(*([-7] * 33))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n0 = lib.rtfs_debug_launch_count()
    rc = lib.rtfs_debug_dw_f32(op, P, len(ptrs), I, len(ints), Dd, len(dbls), R, 33, st)
    launches = lib.rtfs_debug_launch_count() - n0
    return rc, launches, [tuple(R[1 + 8 * i:9 + 8 * i]) for i in range(R[0])]


# ------------------------------------------------------------------------------------------------ comparisons
def same(name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} != {ref.shape}"
    assert ref.dtype == np.int64 and int(np.abs(ref).max(initial=0)) < 2 ** 24
    bad = ~(got.astype(np.float64) == ref)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} elements differ from the integer reference, first at {i}: "
                             f"got {got[i]!r}, want {int(ref[i])}")


def floaty(sec, name, tensor, got, ref64, ref32):
    """Record a float comparison; the section's bar is set and asserted by finish()."""
    got = np.asarray(got)
    assert np.isfinite(got).all(), f"{name} {tensor}: non-finite output"
    FLOAT.setdefault(sec, []).append((name, tensor, rel_err(got, ref64), rel_err(ref32, ref64)))


def stats_close(name, got, y64):
    """(B, 2) statistics of the float64 reference tensor y64: sum at 1e-5 of sum|y|, sumsq at rtol 1e-5."""
    f = y64.reshape(y64.shape[0], -1).double()
    ref = D.stats(y64).numpy()
    assert np.isfinite(got).all(), f"{name}: non-finite statistics"
    d0, b0 = np.abs(got[:, 0] - ref[:, 0]), 1e-5 * f.abs().sum(1).numpy()
    assert (d0 <= b0).all(), f"{name}: sum off by {d0.max():.3e} (bar {b0.min():.3e})"
    d1 = np.abs(got[:, 1] - ref[:, 1]) / ref[:, 1]
    assert (d1 <= 1e-5).all(), f"{name}: sumsq rel {d1.max():.3e} > 1e-5"


def stats_same(name, got, yint):
    f = yint.reshape(yint.shape[0], -1)
    ref = np.stack([f.sum(1), (f * f).sum(1)], 1)
    assert np.array_equal(got, ref.astype(np.float64)), f"{name}: statistics {got.tolist()} != {ref.tolist()}"


def finish(sec):
    """The section's bar from its own float32 restatement, then every recorded case against it."""
    rows = FLOAT.pop(sec, [])
    n = COUNT.get(sec, 0)
    if not rows:
        print(f"[dw] {sec}: {n} cases, exact only")
        return
    f32 = max(r[3] for r in rows)
    bar = 10 * f32
    worst = max(rows, key=lambda r: r[2])
    print(f"[dw] {sec}: {n} cases, {len(rows)} float tensors, float32 restatement worst {f32:.3e}, bar {bar:.3e}, "
          f"worst GPU {worst[2]:.3e} ({worst[0]} {worst[1]})")
    assert bar < 1e-4, f"{sec}: bar {bar:.3e} is not below the project's 1e-4"
    bad = [r for r in rows if not r[2] <= bar]
    assert not bad, f"{sec}: {len(bad)} of {len(rows)} tensors above the bar {bar:.3e}, worst {worst[0]} {worst[1]}: {worst[2]:.3e}"


# ------------------------------------------------------------------------------------------------ the stride-1 launcher, one case
def _gb(rng, C):
    return (1 + 0.2 * rng.standard_normal(C)).astype(np.float32), (0.2 * rng.standard_normal(C)).astype(np.float32)


def s1_case(sec, B, C, H, W, expect, *, nconv=1, in_affine=False, mode=0, TH=8, cs=0, rev=0, Hg=0, Wg=0, addend=False, in_combine=False,
            integer=False, seed=0, out_off=0, launches=1):
    """One launch_dw_s1 call.  expect: the route job tuples.  Returns the outputs (list of (B, C, H, W) float32) and statistics."""
    name = (f"s1 n{nconv} aff{int(in_affine)} m{mode} B{B} C{C} H{H} W{W} TH{TH} cs{cs} rev{rev} g{Hg}x{Wg} add{int(addend)} "
            f"comb{int(in_combine)} off{out_off}")
    COUNT[sec] = COUNT.get(sec, 0) + 1
    assert not integer or not (in_affine or mode == 2 or in_combine)
    rng = np.random.default_rng([seed, B, C, H, W, mode, nconv])
    draw = (lambda s, lo=-2, hi=2: rng.integers(lo, hi + 1, s).astype(np.float32)) if integer else \
           (lambda s, lo=0, hi=0: rng.standard_normal(s).astype(np.float32))
    csz = cs or H * W
    x = draw((B, C, H, W))
    w = [draw((C, 16)) if integer else (0.3 * rng.standard_normal((C, 16))).astype(np.float32) for _ in range(nconv)]
    bias = [None] * nconv if mode == 2 or in_combine else [draw((C,), -1, 1) for _ in range(nconv)]
    k = dict(B=B, C=C, H=H, W=W, Hg=Hg, Wg=Wg, TH=TH, cs=cs, rev=rev, nconv=nconv, in_affine=in_affine, mode=mode, in_combine=in_combine)
    keep = []  # device tensors stay alive until the call is done
    def d(a, dtype=np.float32):
        keep.append(dv(a, dtype))
        return keep[-1]
    k["x"] = strided(x, csz)
    k["w"] = [d(v) for v in w]
    k["bias"] = [None if v is None else d(v) for v in bias]
    x64 = D.t64(x)
    ref = {}  # dtype -> list of output tensors
    fold_in = gate = emb = add = None
    if in_affine:
        fold_in = (D.stats(x64), *_gb(rng, C))
        k.update(in_stats=d(fold_in[0].numpy(), np.float64), in_gamma=d(fold_in[1]), in_beta=d(fold_in[2]), in_inv=1.0 / (C * H * W))
    if in_combine or mode == 2:
        gs = (B, C, H, W) if in_combine else (B, C, Hg, Wg)
        gate, emb = draw(gs), draw(gs)
        lgb, ggb, egb = _gb(rng, C), _gb(rng, C), _gb(rng, C)
        gst, est = D.stats(D.t64(gate)), D.stats(D.t64(emb))
        k.update(gate=d(gate), emb=d(emb), gate_stats=d(gst.numpy(), np.float64), emb_stats=d(est.numpy(), np.float64),
                 gate_gamma=d(ggb[0]), gate_beta=d(ggb[1]), emb_gamma=d(egb[0]), emb_beta=d(egb[1]), loc_gamma=d(lgb[0]), loc_beta=d(lgb[1]),
                 g_inv=1.0 / (C * gs[2] * gs[3]))
    if addend:
        add = draw((B, C, H, W))
        agb, ast = _gb(rng, C), D.stats(D.t64(add))
        k.update(addend=strided(add, csz), add_stats=d(ast.numpy(), np.float64), add_gamma=d(agb[0]), add_beta=d(agb[1]), add_inv=1.0 / (C * H * W))

    def conv_input(dt):
        xx = torch.as_tensor(x).to(dt)
        if in_affine:
            return D.fold(xx, *fold_in)
        if in_combine:
            return D.combine(xx, D.stats(x64), lgb, torch.as_tensor(gate).to(dt), gst, ggb, torch.as_tensor(emb).to(dt), est, egb)
        return xx
    if in_combine:
        k["loc_stats"] = d(D.stats(x64).numpy(), np.float64)
    if mode == 2:
        lst = D.stats(D.conv_s1(conv_input(torch.float64), w[0]))
        k.update(loc_stats=d(lst.numpy(), np.float64), loc_inv=1.0 / (C * H * W))

    def reference(dt):
        xin = conv_input(dt)
        if mode == 2:
            return [D.apply(xin, w[0], lst, lgb, torch.as_tensor(gate).to(dt), gst, ggb, torch.as_tensor(emb).to(dt), est, egb,
                            None if add is None else torch.as_tensor(add).to(dt), None if add is None else ast, None if add is None else agb)]
        return [D.conv_s1(xin, w[n], bias[n]) for n in range(nconv)]
    if integer:
        ref64 = reference(torch.int64)
    else:
        ref64, ref32 = reference(torch.float64), reference(torch.float32)
    outs = [_out(B * C * csz + out_off) for _ in range(nconv)] if mode != 1 else []
    sts = [_stats_buf(B) for _ in range(nconv)] if mode != 2 else []
    k["out"] = [t[out_off:] for t in outs]
    k["stats_out"] = sts
    rc, n, route = call(0, desc(**k))
    assert rc == 0, f"{name}: status {rc}"
    assert route == list(expect), f"{name}: route {route}, expected {list(expect)}"
    assert n == launches, f"{name}: {n} launches"
    got = [unstrided(_take(t, B * C * csz + out_off, name)[out_off:], B, C, H, W, csz) for t in outs]
    gst_ = [_take_stats(t, B, name) for t in sts]
    for i, g in enumerate(got):
        if integer:
            same(f"{name} out[{i}]", g, ref64[i].numpy())
        else:
            floaty(sec, name, f"out[{i}]", g, ref64[i].numpy(), ref32[i].numpy())
    for i, g in enumerate(gst_):
        if integer:
            stats_same(f"{name} stats[{i}]", g, ref64[i].numpy())
        else:
            stats_close(f"{name} stats[{i}]", g, ref64[i])
    return got, gst_


# ------------------------------------------------------------------------------------------------ 1. band edges
BAND_H = lambda TH: sorted({1, 2, 3, 4, 5, TH - 1, TH, TH + 1, TH + 2, TH + 3, 2 * TH - 1, 2 * TH, 2 * TH + 3})


@pytest.mark.parametrize("TH", [8, 24, 64])
def test_band_edges_packed_single_conv(TH):
    """MODE 0 / 1 / 2 with and without the input fold at W = 33, H around every multiple of the band.  At B = 1 and 3 a launch is far below
    512 workgroups, so the effective band is band_rows()' shortened one: that is what the route assertion pins (768-workgroup target for
    MODE 2, 320 for the launches that end in statistics atomics)."""
    sec = f"1 band edges TH {TH}"
    C, W = 4, 33
    for H, B, aff in itertools.product(BAND_H(TH), (1, 3), (False, True)):
        s1_case(sec, B, C, H, W, [packed(1, aff, 0, 0, B, C, H, W, TH)], in_affine=aff, mode=0, TH=TH, integer=not aff)
        s1_case(sec, B, C, H, W, [packed(1, aff, 1, 0, B, C, H, W, TH)], in_affine=aff, mode=1, TH=TH, integer=not aff)
        Hg = max(1, H // 2)
        assert not departs(Hg, H) and not departs(16, W)
        s1_case(sec, B, C, H, W, [packed(1, aff, 2, SHARE, B, C, H, W, TH)], in_affine=aff, mode=2, TH=TH, Hg=Hg, Wg=16)
    finish(sec)


def test_band_edges_at_the_full_band_height():
    """The same edges where the requested band survives: with one workgroup per band and sample, 512 workgroups take a batch of 256 at two
    bands.  H mod 24 in {23, 0, 1, 2, 3}: the last whole band is the one whose `border` flag decides about the rows behind the image."""
    sec = "1b band edges, 24-row bands"
    C, W, TH = 4, 33, 24
    for H in (47, 48, 49, 50, 51):
        B = cdiv(512, cdiv(H, TH))
        assert packed(1, False, 0, 0, B, C, H, W, TH)[5] == TH and packed(1, True, 2, SHARE, B, C, H, W, TH)[5] == TH
        s1_case(sec, B, C, H, W, [packed(1, False, 0, 0, B, C, H, W, TH)], TH=TH, integer=True)
        s1_case(sec, B, C, H, W, [packed(1, True, 2, SHARE, B, C, H, W, TH)], in_affine=True, mode=2, TH=TH, Hg=H // 2, Wg=16)
    finish(sec)


# ------------------------------------------------------------------------------------------------ 2. band_rows on both sides of its switch
def test_band_rows_switch():
    """C = 64, W = 129: one (B, H) just below and one just above gx gy B = 512 for the 24-row bands of the write and apply passes (row
    mapping, gx = 16), the 64-row bands of the statistics pass and the 12-row bands of the stride-2 pass (gx = 17)."""
    sec = "2 band_rows switch"
    C, W = 64, 129
    for H, th in ((72, 16), (73, 24)):  # 16 * 3 * 8 = 384 -> the apply pass shortens to 16; 16 * 4 * 8 = 512 -> 24 kept
        B, cs = 8, pitch(H * W)
        e = packed(1, False, 0, ROW, B, C, H, W, 24)
        assert e[5] == 24  # (the 320-workgroup target of the write pass asks for 3 bands below the switch: 24 rows either way)
        s1_case(sec, B, C, H, W, [e], TH=24, cs=cs, integer=True)
        e = packed(1, True, 2, ROW | SHARE, B, C, H, W, 24)
        assert e[5] == th
        s1_case(sec, B, C, H, W, [e], in_affine=True, mode=2, TH=24, cs=cs, Hg=H // 2, Wg=64)
    for H, th in ((64, 32), (65, 64)):  # 17 * 1 * 16 = 272 -> 32-row bands; 17 * 2 * 16 = 544 -> 64 kept, second band one row
        e = packed(1, False, 1, 0, 16, C, H, W, 64)
        assert e[5] == th
        s1_case(sec, 16, C, H, W, [e], mode=1, TH=64, integer=True)
    for H, th in ((24, 8), (26, 12)):  # Ho = 12: 272 workgroups -> 8; Ho = 13: 544 -> 12 kept
        e = s2_case(sec, 16, C, H, W, pool_only=True, TH=12)
        assert e[0][5] == th, e
    finish(sec)


# ------------------------------------------------------------------------------------------------ 3. width and mapping edges
WIDTHS = [16, 17, 31, 32, 33, 63, 64, 65] + list(range(121, 132))


@pytest.mark.parametrize("C", [4, 8, 64])
def test_width_edges(C):
    """H = 11: 61 / 62 / 63 pairs per row and waves that straddle channel boundaries at every offset, the odd last pair (x1 == W), the
    `gi < C NP` tail in the last wave, and the row mapping at W = 129 (contiguous planes qualify when H W % 32 == 0 does not: H = 11 is
    the non-row route, so W = 129 runs both: cs = 0 and cs = pitch)."""
    sec = f"3 width edges C {C}"
    H, B = 11, 2
    for W in WIDTHS:
        Wg = W // 2
        assert not departs(Wg, W) and not departs(5, H)
        s1_case(sec, B, C, H, W, [packed(1, False, 0, 0, B, C, H, W, 8)], integer=True)
        s1_case(sec, B, C, H, W, [packed(1, False, 2, SHARE | ADD, B, C, H, W, 8)], mode=2, Hg=5, Wg=Wg, addend=True)
        s1_case(sec, B, C, H, W, [packed(1, True, 2, SHARE, B, C, H, W, 8)], in_affine=True, mode=2, Hg=5, Wg=Wg)
    W, cs = 129, pitch(H * 129)
    s1_case(sec, B, C, H, W, [packed(1, False, 0, ROW, B, C, H, W, 8)], cs=cs, integer=True)
    s1_case(sec, B, C, H, W, [packed(1, False, 2, ROW | SHARE | ADD, B, C, H, W, 8)], mode=2, cs=cs, Hg=5, Wg=64, addend=True)
    s1_case(sec, B, C, H, W, [packed(1, True, 2, ROW | SHARE, B, C, H, W, 8)], in_affine=True, mode=2, cs=cs, Hg=5, Wg=64)
    finish(sec)


# ------------------------------------------------------------------------------------------------ 4. row variants
@pytest.mark.parametrize("B", [1, 3])
def test_row_variants(B):
    """VAR 8 / 10 / 11 (W = 129, cs % 32 == 0, 128-byte-aligned output).  With cs = pitch(H 129) and 516-byte rows the ring's 512-byte chunks
    end at every alignment against a band's last row; Wg in {64, 43, 17} moves the shared-gather columns and lane 0's gather."""
    sec = f"4 row variants B {B}"
    C, W = 4, 129
    for H in (8, 9, 15, 16, 17, 31, 32, 33):
        cs = pitch(H * W)
        s1_case(sec, B, C, H, W, [packed(1, False, 0, ROW, B, C, H, W, 24)], TH=24, cs=cs, integer=True)
        for Wg in (64, 43, 17):
            assert not departs(H // 2, H) and not departs(Wg, W)
            s1_case(sec, B, C, H, W, [packed(1, True, 2, ROW | SHARE, B, C, H, W, 24)], in_affine=True, mode=2, TH=24, cs=cs, Hg=H // 2, Wg=Wg)
            s1_case(sec, B, C, H, W, [packed(1, False, 2, ROW | SHARE | ADD, B, C, H, W, 24)], mode=2, TH=24, cs=cs, Hg=H // 2, Wg=Wg,
                    addend=True, rev=1)
    # contiguous planes: H = 32 qualifies (32 * 129 % 32 == 0), H = 17 must report the non-row route; so must an output 64 bytes off a line,
    # and the two MODE 2 forms the row mapping has no variant for
    s1_case(sec, B, C, 32, W, [packed(1, False, 0, ROW, B, C, 32, W, 24)], TH=24, integer=True)
    s1_case(sec, B, C, 32, W, [packed(1, True, 2, ROW | SHARE, B, C, 32, W, 24)], in_affine=True, mode=2, TH=24, Hg=16, Wg=64)
    s1_case(sec, B, C, 17, W, [packed(1, False, 0, 0, B, C, 17, W, 24)], TH=24, integer=True)
    s1_case(sec, B, C, 17, W, [packed(1, True, 2, SHARE, B, C, 17, W, 24)], in_affine=True, mode=2, TH=24, Hg=8, Wg=64)
    s1_case(sec, B, C, 32, W, [packed(1, False, 0, 0, B, C, 32, W, 24)], TH=24, integer=True, out_off=16)
    s1_case(sec, B, C, 32, W, [packed(1, True, 2, SHARE, B, C, 32, W, 24)], in_affine=True, mode=2, TH=24, Hg=16, Wg=64, out_off=16)
    s1_case(sec, B, C, 32, W, [packed(1, True, 2, SHARE | ADD, B, C, 32, W, 24)], in_affine=True, mode=2, TH=24, Hg=16, Wg=64, addend=True)
    s1_case(sec, B, C, 32, W, [packed(1, False, 2, SHARE, B, C, 32, W, 24)], mode=2, TH=24, Hg=16, Wg=64)
    s1_case(sec, B, C, 32, W, [packed(1, True, 0, 0, B, C, 32, W, 24)], in_affine=True, TH=24)
    finish(sec)


# ------------------------------------------------------------------------------------------------ 5. MODE 2 variants
def test_mode2_variants():
    """VAR 0 - 3: addend x (2 Wg <= W), with and without the input fold, on agreeing pairs; H in {2 Hg, 2 Hg + 1} for the incremental row
    quotient; the departing pair (14, 26) -> (46, 44) must report the one-column kernel."""
    sec = "5 MODE 2 variants"
    C = 8
    table = [(9, 33, 9, 33), (10, 33, 5, 16), (11, 33, 5, 16), (17, 33, 5, 8), (10, 33, 5, 8), (11, 33, 5, 8), (10, 33, 5, 20), (11, 33, 5, 20),
             (16, 64, 8, 32), (17, 64, 8, 33)]
    for (H, W, Hg, Wg), add, aff, B in itertools.product(table, (False, True), (False, True), (1, 3)):
        assert not departs(Hg, H) and not departs(Wg, W)
        var = (ADD if add else 0) | (SHARE if 2 * Wg <= W else 0)
        s1_case(sec, B, C, H, W, [packed(1, aff, 2, var, B, C, H, W, 24)], in_affine=aff, mode=2, TH=24, Hg=Hg, Wg=Wg, addend=add)
    assert {(2 * Wg <= W) for _, W, _, Wg in table} == {True, False}
    assert departs(14, 46) and departs(26, 44)
    for add, aff in itertools.product((False, True), (False, True)):
        s1_case(sec, 2, 4, 46, 44, [onecol(1, aff, 2, 4, 46, 44, 24)], in_affine=aff, mode=2, TH=24, Hg=14, Wg=26, addend=add)
    finish(sec)


# ------------------------------------------------------------------------------------------------ 6. multi-conv, combine, g3, one-column
def test_multi_conv_and_combined_input():
    sec = "6 multi-conv and combine"
    C, H = 8, 11
    for B in (1, 3):
        s1_case(sec, B, C, H, 33, [packed(2, False, 0, 0, B, C, H, 33, 64)], nconv=2, TH=64, integer=True)
        s1_case(sec, B, C, H, 64, [packed(2, False, 0, 0, B, C, H, 64, 64)], nconv=2, TH=64, integer=True)
        # the 4-conv request is two 2-conv launches
        e = packed(2, False, 0, 0, B, C, H, 33, 64)
        s1_case(sec, B, C, H, 33, [e, e], nconv=4, TH=64, integer=True, launches=2)
        # the combined input: whole rows per wave where the pair count divides 64, the halo mapping otherwise
        for W in (16, 31, 32, 63, 64, 127, 128):
            s1_case(sec, B, C, H, W, [packed(2, False, 0, COMB | NOHALO, B, C, H, W, 64)], nconv=2, TH=64, in_combine=True)
        for W in (17, 33, 65, 129):
            s1_case(sec, B, C, H, W, [packed(2, False, 0, COMB, B, C, H, W, 64)], nconv=2, TH=64, in_combine=True)
        for Hh in (63, 64, 65):
            s1_case(sec, B, C, Hh, 64, [packed(2, False, 0, COMB | NOHALO, B, C, Hh, 64, 64)], nconv=2, TH=64, in_combine=True)
    finish(sec)


def test_narrow_combine_route_of_the_block():
    """W = 12 as block_body runs it: launch_g_combine writes xf1, then the plain 2-conv launch (one-column kernel) reads it."""
    sec = "6 narrow combine"
    B, C, H, W = 2, 8, 9, 12
    COUNT[sec] = 1
    rng = np.random.default_rng(12)
    l, gate, emb = (rng.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(3))
    gbs = [_gb(rng, C) for _ in range(3)]
    sts = [D.stats(D.t64(v)) for v in (l, gate, emb)]
    w = [(0.3 * rng.standard_normal((C, 16))).astype(np.float32) for _ in range(2)]
    xf = {dt: D.combine(torch.as_tensor(l).to(dt), sts[0], gbs[0], torch.as_tensor(gate).to(dt), sts[1], gbs[1], torch.as_tensor(emb).to(dt),
                        sts[2], gbs[2]) for dt in (torch.float64, torch.float32)}
    xf1 = _out(B * C * H * W)
    keep = [dv(v) for v in (l, gate, emb)] + [dv(s.numpy(), np.float64) for s in sts] + [dv(v) for gb in gbs for v in gb]
    rc, n, route = call(5, flat=([t.data_ptr() for t in keep] + [xf1.data_ptr()], [B, C, H * W], [1.0 / (C * H * W)]))
    assert (rc, n, route) == (0, 1, [(GCOMBINE, 0, 1, 0, 0, 0, 4, C)]), (rc, n, route)
    got = _take(xf1, B * C * H * W, "xf1").reshape(B, C, H, W)
    floaty(sec, "g_combine W 12", "xf1", got, xf[torch.float64].numpy(), xf[torch.float32].numpy())
    outs, stb, wd = [_out(B * C * H * W) for _ in range(2)], [_stats_buf(B) for _ in range(2)], [dv(v) for v in w]
    rc, n, route = call(0, desc(B=B, C=C, H=H, W=W, TH=64, nconv=2, x=xf1, w=wd, out=outs, stats_out=stb))
    assert (rc, n, route) == (0, 1, [onecol(2, False, 0, C, H, W, 64)]), (rc, n, route)
    for i in range(2):
        # the conv's own reference starts from the tensor the kernel read (the combine's error is the line above)
        r64, r32 = D.conv_s1(D.t64(got), w[i]), D.conv_s1(torch.as_tensor(got), w[i])
        floaty(sec, "2-conv on xf1", f"out[{i}]", _take(outs[i], B * C * H * W, "E2/G2").reshape(B, C, H, W), r64.numpy(), r32.numpy())
        stats_close(f"2-conv on xf1 stats[{i}]", _take_stats(stb[i], B, "stats"), r64)
    finish(sec)


def g3_case(sec, B, C, H, W, rev=0):
    """launch_dw_g3: jobs 0 / 1 (four plain convs on one input, exact integers) and job 2 (one conv on a folded input, float)."""
    name = f"g3 B{B} C{C} H{H} W{W}"
    COUNT[sec] = COUNT.get(sec, 0) + 1
    rng = np.random.default_rng([3, B, C, H, W])
    x = rng.integers(-2, 3, (B, C, H, W)).astype(np.float32)
    w4 = [rng.integers(-2, 3, (C, 16)).astype(np.float32) for _ in range(4)]
    b4 = [rng.integers(-1, 2, (C,)).astype(np.float32) for _ in range(4)]
    x2 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    w1 = (0.3 * rng.standard_normal((C, 16))).astype(np.float32)
    gb, st2 = _gb(rng, C), D.stats(D.t64(x2))
    keep = [dv(x), dv(x2), dv(w1), dv(st2.numpy(), np.float64), dv(gb[0]), dv(gb[1])] + [dv(v) for v in w4] + [dv(v) for v in b4]
    outs, sts = [_out(B * C * H * W) for _ in range(5)], [_stats_buf(B) for _ in range(5)]
    a = desc(B=B, C=C, H=H, W=W, TH=64, nconv=4, rev=rev, x=keep[0], w=keep[6:10], bias=keep[10:14], out=outs[:4], stats_out=sts[:4])
    l = desc(B=B, C=C, H=H, W=W, TH=64, in_affine=True, rev=rev, x=keep[1], w=[keep[2]], in_stats=keep[3], in_gamma=keep[4], in_beta=keep[5],
             in_inv=1.0 / (C * H * W), out=[outs[4]], stats_out=[sts[4]])
    rc, n, route = call(1, a, l)
    if W < 16:
        assert (rc, n, route) == (ERR_ARG, 0, []), (name, rc, n, route)
        for t in outs:
            _untouched(t, B * C * H * W, name)
        assert all(np.array_equal(_take_stats(t, B, name), np.zeros((B, 2))) for t in sts)
        return
    var = NOHALO if 64 % ((W + 1) // 2) == 0 else 0
    gx = gx_packed(C, W, var)
    th = band_rows(64, H, gx, 3 * B, 640)
    want = [(G3, 2, 0, 0, var, th, gx, cdiv(H, th))] * 2 + [(G3, 1, 1, 0, var, th, gx, cdiv(H, th))]
    assert (rc, n, route) == (0, 1, want), (name, rc, n, route, want)
    for i in range(4):
        r = D.conv_s1(torch.as_tensor(x).long(), torch.as_tensor(w4[i]).long(), torch.as_tensor(b4[i]).long()).numpy()
        same(f"{name} out[{i}]", _take(outs[i], B * C * H * W, name).reshape(B, C, H, W), r)
        stats_same(f"{name} stats[{i}]", _take_stats(sts[i], B, name), r)
    r64, r32 = (D.conv_s1(D.fold(torch.as_tensor(x2).to(dt), st2, *gb), w1) for dt in (torch.float64, torch.float32))
    floaty(sec, name, "L1", _take(outs[4], B * C * H * W, name).reshape(B, C, H, W), r64.numpy(), r32.numpy())
    stats_close(f"{name} stats L1", _take_stats(sts[4], B, name), r64)


def test_three_job_launch():
    """dw_g3 at W = 64 (<16>: whole rows per wave) and W = 33 (<0>), H around the 64-row band; RTFS_ERR_ARG and no launch at W = 12."""
    sec = "6 three-job launch"
    for W, H, B in itertools.product((64, 33), (8, 63, 64, 65), (1, 3)):
        g3_case(sec, B, 8, H, W)
    g3_case(sec, 2, 8, 9, 12)
    g3_case(sec, 3, 8, 65, 33, rev=1)  # the launch has no back-to-front order: the launcher ignores the flag
    finish(sec)


def test_one_column_forms():
    """dw_s1_kernel with NCONV 1 - 4 at W in {1, 2, 3, 5, 15} (exact), NCONV 3 at a packed width (no packed 3-conv form: it reports the
    one-column kernel), and the folded / statistics / apply instantiations."""
    sec = "6 one-column forms"
    B, C = 2, 4
    for W, H, nconv in itertools.product((1, 2, 3, 5, 15), (1, 7, 9), (1, 2, 3, 4)):
        s1_case(sec, B, C, H, W, [onecol(nconv, False, 0, C, H, W, 8)], nconv=nconv, integer=True)
    s1_case(sec, B, C, 9, 33, [onecol(3, False, 0, C, 9, 33, 8)], nconv=3, integer=True)
    for W, H in ((5, 9), (15, 7)):
        s1_case(sec, B, C, H, W, [onecol(1, False, 1, C, H, W, 8)], mode=1, integer=True)
        s1_case(sec, B, C, H, W, [onecol(1, True, 0, C, H, W, 8)], in_affine=True)
        s1_case(sec, B, C, H, W, [onecol(1, True, 1, C, H, W, 8)], in_affine=True, mode=1)
        assert not departs(H // 2, H) and not departs(W // 2, W)
        for aff, add in itertools.product((False, True), (False, True)):
            s1_case(sec, B, C, H, W, [onecol(1, aff, 2, C, H, W, 8)], in_affine=aff, mode=2, Hg=H // 2, Wg=W // 2, addend=add)
    finish(sec)


# ------------------------------------------------------------------------------------------------ 7. stride 2 + pool
def s2_case(sec, B, C, H, W, *, pool_only, TH=12, rev=0, cs=0):
    """launch_dw_s2_pool (pool_only) or launch_dw_s2_stats: c1 and its statistics, p0, and the second job's MODE 1 statistics.  Ho = H // 2,
    Wo = W // 2.  Returns the route."""
    Ho, Wo = H // 2, W // 2
    name = f"s2 {'pool' if pool_only else 'stats'} B{B} C{C} H{H} W{W} rev{rev} cs{cs}"
    COUNT[sec] = COUNT.get(sec, 0) + 1
    rng = np.random.default_rng([7, B, C, H, W])
    csz = cs or H * W
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    w = (0.3 * rng.standard_normal((C, 16))).astype(np.float32)
    wl = (0.3 * rng.standard_normal((C, 16))).astype(np.float32)
    bias = (0.3 * rng.standard_normal(C)).astype(np.float32)
    gb, st = _gb(rng, C), D.stats(D.t64(x))
    keep = [strided(x, csz), dv(st.numpy(), np.float64), dv(gb[0]), dv(gb[1]), dv(w), dv(bias), dv(wl)]
    c1, p0, sc1, sl = _out(B * C * Ho * Wo), _out(B * C * Ho * Wo), _stats_buf(B), _stats_buf(B)
    common = dict(B=B, C=C, H=H, W=W, Hg=Ho, Wg=Wo, cs=cs, x=keep[0], in_stats=keep[1], in_gamma=keep[2], in_beta=keep[3], in_affine=True,
                  in_inv=1.0 / (C * H * W))
    a = desc(TH=TH, rev=rev, w=[keep[4]], bias=[keep[5]], out=[c1, p0], stats_out=[sc1], **common)
    packed_ok = Wo >= 16
    gx = gx_packed(C, W)
    th = band_rows(TH, Ho, gx, B, 320)
    if pool_only:
        rc, n, route = call(3, a)
        want = [(S2X, 1, 1, 0, 0, th, gx, cdiv(Ho, th))] if packed_ok else [(S2POOL, 1, 1, 0, 0, TH, cdiv(C * Wo, 256), cdiv(Ho, TH))]
    else:
        b = desc(TH=64, rev=rev, mode=1, w=[keep[6]], stats_out=[sl], **common)
        rc, n, route = call(2, a, b)
        if not packed_ok:  # not eligible: the caller gets RTFS_ERR_ARG and nothing has run
            assert (rc, n, route) == (ERR_ARG, 0, []), (name, rc, n, route)
            _untouched(c1, B * C * Ho * Wo, name), _untouched(p0, B * C * Ho * Wo, name)
            return route
        ths = band_rows(64, H, gx, B, 320)
        want = [(S2STATS, 1, 1, 0, 0, th, gx, cdiv(Ho, th)), (S2STATS, 1, 1, 1, 0, ths, gx, cdiv(H, ths))]
    assert (rc, n, route) == (0, 1, want), (name, rc, n, route, want)
    refs = {}
    for dt in (torch.float64, torch.float32):
        d0 = D.fold(torch.as_tensor(x).to(dt), st, *gb)
        refs[dt] = D.s2_pool(d0, w, bias, (Ho, Wo)) + (D.conv_s1(d0, wl),)
    for t, tag, i in ((c1, "c1", 0), (p0, "p0", 1)):
        floaty(sec, name, tag, _take(t, B * C * Ho * Wo, name).reshape(B, C, Ho, Wo), refs[torch.float64][i].numpy(), refs[torch.float32][i].numpy())
    stats_close(f"{name} stats c1", _take_stats(sc1, B, name), refs[torch.float64][0])
    if not pool_only:
        stats_close(f"{name} stats L0", _take_stats(sl, B, name), refs[torch.float64][2])
    return route


S2_H = (16, 17, 23, 24, 25, 26, 27, 48, 49)


@pytest.mark.parametrize("W", [32, 33, 129])
def test_stride2_pool_packed(W):
    """dw_s2x alone and beside the statistics job: pool windows of 2 and 3 rows / columns, the dead slot j = Wo of odd widths, bands with an
    odd number of output rows, both traversal orders, B in {1, 2, 3} for the per-sample interleaving of the two jobs."""
    sec = f"7 stride 2 packed W {W}"
    for H, B, rev in itertools.product(S2_H, (1, 2, 3), (0, 1)):
        s2_case(sec, B, 4, H, W, pool_only=True, rev=rev)
        s2_case(sec, B, 4, H, W, pool_only=False, rev=rev)
    s2_case(sec, 2, 8, 25, W, pool_only=False, rev=1, cs=pitch(25 * W))
    finish(sec)


def test_stride2_pool_one_column():
    sec = "7 stride 2 one-column"
    for H, W, B in itertools.product(S2_H, (4, 5, 30), (1, 2, 3)):
        s2_case(sec, B, 4, H, W, pool_only=True)
    s2_case(sec, 2, 4, 17, 30, pool_only=False)  # Wo = 15: the two-job launch is not eligible
    finish(sec)


# ------------------------------------------------------------------------------------------------ 8. rev and launch padding
def test_rev_and_launch_padding():
    """nblk % 8 in {0, 1, 7}: the 1-D launch is padded to a multiple of 8 and every XCD eighth walks its blocks front to back or back to
    front.  Outputs of rev = 1 are bit-identical to rev = 0; statistics (atomics reorder) are held to the float bars by s1_case."""
    sec = "8 rev and launch padding"
    C, W = 4, 33
    for H, B in ((64, 1), (65, 1), (56, 1), (64, 3), (24, 3), (40, 3)):
        e0, e2 = packed(1, True, 0, 0, B, C, H, W, 8), packed(1, True, 2, SHARE | ADD, B, C, H, W, 8)
        assert (e0[6] * e0[7] * B) % 8 in (0, 1, 7) and (e2[6] * e2[7] * B) % 8 in (0, 1, 7)
        r = [s1_case(sec, B, C, H, W, [e0], in_affine=True, rev=rev) for rev in (0, 1)]
        assert np.array_equal(r[0][0][0].view(np.uint32), r[1][0][0].view(np.uint32)), f"MODE 0 H{H} B{B}: rev changes the output"
        r = [s1_case(sec, B, C, H, W, [e2], in_affine=True, mode=2, Hg=H // 2, Wg=16, addend=True, rev=rev) for rev in (0, 1)]
        assert np.array_equal(r[0][0][0].view(np.uint32), r[1][0][0].view(np.uint32)), f"MODE 2 H{H} B{B}: rev changes the output"
    assert {(packed(1, True, 0, 0, B, C, H, W, 8)[7] * B) % 8 for H, B in ((64, 1), (65, 1), (56, 1), (64, 3), (24, 3), (40, 3))} == {0, 1, 7}
    finish(sec)


# ------------------------------------------------------------------------------------------------ 9. g_form and g_combine
@pytest.mark.parametrize("C,Bs", [(4, (2, 255, 256)), (64, (15, 16))])
def test_g_form_and_g_combine(C, Bs):
    """HW in {1, 255, 256, 257, 1023} (the 16-byte form needs HW % 4 == 0) on both sides of the B C >= 1024 grid switch."""
    sec = f"9 g_form and g_combine C {C}"
    for HW, B in itertools.product((1, 255, 256, 257, 1023), Bs):
        COUNT[sec] = COUNT.get(sec, 0) + 2
        rng = np.random.default_rng([9, C, HW, B])
        t = [rng.standard_normal((B, C, HW)).astype(np.float32) for _ in range(3)]
        gbs, sts = [_gb(rng, C) for _ in range(3)], [D.stats(D.t64(v)) for v in t]
        gx = 1 if B * C >= 1024 else 4
        td, sd, gd = [dv(v) for v in t], [dv(s.numpy(), np.float64) for s in sts], [dv(v) for gb in gbs for v in gb]
        g = _out(B * C * HW)
        rc, n, route = call(4, flat=([td[0].data_ptr(), td[1].data_ptr(), sd[1].data_ptr(), gd[2].data_ptr(), gd[3].data_ptr(), g.data_ptr()],
                                     [B, C, HW], [1.0 / (C * HW)]))
        assert (rc, n, route) == (0, 1, [(GFORM, 0, 1, 0, 0, 0, gx, C)]), (rc, n, route)
        r = [D.g_form(torch.as_tensor(t[0]).to(dt), torch.as_tensor(t[1]).to(dt), sts[1], gbs[1]).numpy() for dt in (torch.float64, torch.float32)]
        floaty(sec, f"g_form B{B} HW{HW}", "g", _take(g, B * C * HW, "g").reshape(B, C, HW), *r)
        o = _out(B * C * HW)
        rc, n, route = call(5, flat=([v.data_ptr() for v in td + sd + gd] + [o.data_ptr()], [B, C, HW], [1.0 / (C * HW)]))
        assert (rc, n, route) == (0, 1, [(GCOMBINE, 0, 1, 0, 0, 0, gx, C)]), (rc, n, route)
        r = [D.combine(torch.as_tensor(t[0]).to(dt), sts[0], gbs[0], torch.as_tensor(t[1]).to(dt), sts[1], gbs[1], torch.as_tensor(t[2]).to(dt),
                       sts[2], gbs[2]).numpy() for dt in (torch.float64, torch.float32)]
        floaty(sec, f"g_combine B{B} HW{HW}", "out", _take(o, B * C * HW, "out").reshape(B, C, HW), *r)
    finish(sec)


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals():
    """Every documented refusal returns its code, launches nothing, records no route and writes nothing."""
    B, C, H, W = 2, 4, 9, 33
    x, wt, out, st = dv(np.zeros((B, C, H, W))), dv(np.zeros((C, 16))), _out(B * C * H * W), _stats_buf(B)
    out2 = _out(B * C * H * W)
    gam = dv(np.ones(C))
    base = dict(B=B, C=C, H=H, W=W, x=x, w=[wt] * 4, out=[out, out2, out, out2], stats_out=[st] * 4)
    aff = dict(in_affine=True, in_stats=st, in_gamma=gam, in_beta=gam, in_inv=1.0, Hg=H // 2, Wg=W // 2)
    def refused(code, op, *descs):
        rc, n, route = call(op, *descs)
        assert (rc, n, route) == (code, 0, []), (op, rc, n, route)
        _untouched(out, B * C * H * W, f"op {op}"), _untouched(out2, B * C * H * W, f"op {op}")
        assert np.array_equal(_take_stats(st, B, "stats"), np.zeros((B, 2)))
    # cs < H W
    refused(ERR_SHAPE, 0, desc(cs=H * W - 1, **base))
    refused(ERR_SHAPE, 3, desc(cs=H * W - 1, **base, **aff))
    refused(ERR_ARG, 1, desc(cs=H * W - 1, nconv=4, **base), desc(**base, **aff))
    refused(ERR_ARG, 2, desc(cs=H * W - 1, **base, **aff), desc(cs=H * W - 1, mode=1, **base, **aff))
    # the 31-bit span of the lane offsets, C cs 4 >= 2^31: fabricated sizes, nothing that large is allocated (the launchers return before
    # any launch).  launch_dw_s2_pool has no such refusal - its one-column kernel addresses with 64 bits - so it is not called here.
    big = dict(base, C=64, H=65536, W=129)
    assert 64 * 65536 * 129 * 4 >= 2 ** 31
    refused(ERR_SHAPE, 0, desc(**big))
    refused(ERR_SHAPE, 0, desc(mode=1, **big))
    refused(ERR_ARG, 1, desc(nconv=4, **big), desc(**big, **dict(aff, Hg=0, Wg=0)))
    refused(ERR_ARG, 2, desc(**big, **dict(aff, Hg=32768, Wg=64)), desc(mode=1, **big, **dict(aff, Hg=32768, Wg=64)))
    # the two jobs of launch_dw_s2_stats must describe one input
    for k, v in (("H", H + 1), ("W", W + 1), ("C", C + 4), ("cs", pitch(H * W)), ("x", out2)):
        refused(ERR_ARG, 2, desc(**base, **aff), desc(mode=1, **dict(base, **{k: v}), **aff))
    # requests no instantiation serves
    refused(ERR_ARG, 0, desc(nconv=2, mode=1, **base))
    refused(ERR_ARG, 0, desc(nconv=2, **base, **aff))
    # the entry point itself: unknown op, short arrays
    rc, n, route = call(9, desc(**base))
    assert (rc, n, route) == (ERR_ARG, 0, [])
    p, i, d = desc(**base)
    rc, n, route = call(1, (p, i, d))  # one description where op 1 takes two
    assert (rc, n, route) == (ERR_ARG, 0, [])
