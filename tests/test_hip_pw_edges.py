"""Boundary sweeps of the inference pointwise family (csrc/k_pw.hip, k_pw16.hip, k_pwr.hip, k_pws.hip, k_b2b.hip): every launcher, one at a
time, through rtfs_debug_pw_f32, against tests/pw_reference.py, every element compared.  The fused head and tail kernels (k_bnh.hip,
k_s3f.hip) run behind the production launch_enc_stats, as in separator_part.

Routes.  Every case states the route it is meant to take - kernel family, template form, tiles per sample, tiles, workgroups, counter or
static stride - and asserts the record the launcher hands back; a refusal must leave the record empty, launch nothing and write nothing.

Two tiers.
* Exact: every op without a gLN runs on small integers (activations in -3..3, weights in -2..2 so that 256 w is an f16 integer, PReLU slope
  0.5, integer gateway / CAF / BatchNorm constants with sqrt(var + eps) = 1 in float32): no rounding anywhere, so the GPU result must EQUAL
  the float64 reference.  The test checks from the reference's own |W| @ |X| + |addends| that every sum stays below 2^24 units of 1/8.
* Float: random floats (x 16: an activation below 2^-3 loses its flushed f16 lo part by design - DESIGN.md "Range" - which at unit scale is
  the whole error), per element |got - ref64| / (|W| @ |X| + |addends|).  The bar of an op is ten times the worst value of the same measure
  for the CPU emulation of the f16x3 arithmetic (pw_reference.F16X3; float32 torch for the exact-f32 kernels), and never above 1e-5.

Buffers: every output is followed by a guard band that must come back untouched, and the padding of its rows ([P, cs) for the kernels that
take any pitch, [pitch(P), cs) for the padded-row kernels, whose stores are whole 64-pixel wave segments) must keep its bits.  Input
padding is NaN.  No case is meant to fault: every shape satisfies its launcher's preconditions or is one the launcher refuses."""
import ctypes

import numpy as np
import pytest
import torch

from tests import pw_reference as R
from tests.test_hip_parity import host

pytestmark = pytest.mark.gpu

ERR_SHAPE, ERR_ARG = -1, -4
GUARD = 1024
F32K, PW16, PWS, RES2, B2B, B2B4, HEAD4, PWR, BNHEAD, TAIL = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10      # route families (include/rtfs_amd.h)
GLN_RELU, GATEWAY, PRELU = 1, 2, 3                                         # PRO
BIAS, BIAS_RES, S3, TAPS = 0, 1, 2, 3                                      # EPI
PS = [2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 387]
FLOAT_PS = [3, 65, 129, 258, 387]
SCALE = 16.0
FLOAT = {}  # section -> list of (case, tensor, gpu error, emulation error)
COUNT = {}


def cdiv(a, b):
    return -(-a // b)


def pitch(n):
    return (n + 63) // 64 * 64


def _L():
    from rtfs_net_amd import _lib as L
    return L.load(), L


def dv(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


class Buf:
    """A (B, C, cs) device tensor behind which a guard band lies.  `init` (B, C, P) fills the live columns; everything else is NaN (inputs)
    or what _lib.empty gave (outputs: NaN, or the poison of a poisoned run)."""

    def __init__(self, B, C, P, cs, init=None):
        _, L = _L()
        self.B, self.C, self.P, self.cs = B, C, P, cs or P
        self.n = B * C * self.cs
        self.t = L.empty(self.n + GUARD, device="cuda")
        if L._POISON is None or init is not None:
            self.t[:self.n] = float("nan")
        self.t[self.n:] = torch.arange(GUARD, dtype=torch.float32, device="cuda") + 0.5
        if init is not None:
            self.t[:self.n].view(B, C, self.cs)[:, :, :P] = dv(init)
        self.before = host(self.t).copy()

    def ptr(self):
        return self.t.data_ptr()

    def take(self, name, pad_from=None):
        """The live columns after the call; the guard and the columns from `pad_from` (default P) on must have kept their bits."""
        h = host(self.t)
        assert np.array_equal(h[self.n:].view(np.uint32), self.before[self.n:].view(np.uint32)), f"{name}: written past its end"
        a, b = h[:self.n].reshape(self.B, self.C, self.cs), self.before[:self.n].reshape(self.B, self.C, self.cs)
        k = self.P if pad_from is None else pad_from
        assert np.array_equal(a[:, :, k:].view(np.uint32), b[:, :, k:].view(np.uint32)), f"{name}: row padding from column {k} on written"
        return a[:, :, :self.P]

    def untouched(self, name):
        h = host(self.t)
        assert np.array_equal(h.view(np.uint32), self.before.view(np.uint32)), f"{name}: written by a refused call"


def call(op, B, P, cs=0, kind=0, cout_live=0, inv_count=0.0, caf=None, a1_mode=1, xk=1, a1k=1, mix_base=0, tf=(0, 0), nmix=0, **ptrs):
    """-> (status, launches, [route tuples]).  ptrs: name -> Buf, device tensor, or None."""
    names = ("x x2 res_out wt w16 w16b bias aux out stats gamma beta gw gb slope tile_ctr caf_r caf_att caf_w_key caf_bn_key caf_w_val caf_bn_val "
             "caf_rt caf_attt a1 w2_16 bp mix_of spec enc_w enc_img wpad").split()
    assert set(ptrs) <= set(names), set(ptrs) - set(names)
    p = []
    for n in names:
        v = ptrs.get(n)
        p.append(None if v is None else v.ptr() if isinstance(v, Buf) else v.data_ptr())
    T, F, Tv = caf if caf else (0, 0, 0)
    ints = [B, P, cs, cout_live, T, F, Tv, a1_mode, xk, a1k, mix_base, kind, tf[0], tf[1], nmix]
    lib, _ = _L()
    Pp = (ctypes.c_void_p * len(p))(*p)
    I = (ctypes.c_int * len(ints))(*ints)
    Dd = (ctypes.c_double * 1)(inv_count)
    Rt = (ctypes.c_int * 25)(*([-7] * 25))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n0 = lib.rtfs_debug_launch_count()
    rc = lib.rtfs_debug_pw_f32(op, Pp, len(p), I, len(ints), Dd, 1, Rt, 25, st)
    torch.cuda.synchronize()
    launches = lib.rtfs_debug_launch_count() - n0
    return rc, launches, [tuple(Rt[1 + 12 * i:13 + 12 * i]) for i in range(Rt[0])]


def ok(name, res, route, launches=1):
    rc, n, got = res
    assert rc == 0, f"{name}: status {rc}"
    assert got == [route], f"{name}: route {got} != {[route]}"
    assert n == launches, f"{name}: {n} launches"


def refused(name, res, status, *bufs, launches=0):
    """launches: 1 for the fused head / tail ops, whose entry runs launch_enc_stats before the launcher refuses."""
    rc, n, got = res
    assert rc == status and n == launches and got == [], f"{name}: status {rc} (want {status}), {n} launches, route {got}"
    for b in bufs:
        b.untouched(name)


def persistent(family, cin, cout, pro, epi, caf, am, mode, P, B, tile, cap, ctr):
    tps = cdiv(P, tile)
    return (family, cin, cout, pro, epi, caf, am, mode, tps, tps * B, min(tps * B, cap), int(ctr))


def ctr_word():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------ comparisons
def same(name, got, ref, scale):
    """Exact tier: ref is the float64 result on integer data, a multiple of 1/8 with every contributing sum below 2^24 such units."""
    ref, scale = ref.numpy(), scale.numpy()
    assert float(scale.max()) * 8 < 2 ** 24, f"{name}: |W| @ |X| + |addends| reaches {scale.max()}: not exact in float32"
    r8 = np.round(ref * 8)
    assert np.abs(ref * 8 - r8).max() < 1e-6, f"{name}: the reference is not a multiple of 1/8"
    ref = r8 / 8
    assert got.shape == ref.shape, f"{name}: shape {got.shape} != {ref.shape}"
    bad = ~(got.astype(np.float64) == ref)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} elements differ from the exact reference, first at {i}: got {got[i]!r}, want {ref[i]!r}")


def floaty(sec, name, tensor, got, ref, scale, emu):
    assert np.isfinite(got).all(), f"{name} {tensor}: non-finite output"
    FLOAT.setdefault(sec, []).append((name, tensor, R.err(got, ref, scale), R.err(emu, ref, scale)))


def finish(sec, what="f16x3 emulation"):
    rows = FLOAT.pop(sec, [])
    n = COUNT.pop(sec, 0)
    MEMO.clear()
    if not rows:
        print(f"[pw] {sec}: {n} cases, exact only")
        return
    emu = max(r[3] for r in rows)
    bar = min(10 * emu, 1e-5)
    worst = max(rows, key=lambda r: r[2])
    print(f"[pw] {sec}: {n} cases, {len(rows)} float tensors, {what} worst {emu:.3e}, bar {bar:.3e}, worst GPU {worst[2]:.3e} ({worst[0]} {worst[1]})")
    assert emu > 0
    bad = [r for r in rows if not r[2] <= bar]
    assert not bad, f"{sec}: {len(bad)} of {len(rows)} tensors above the bar {bar:.3e}, worst {worst[0]} {worst[1]}: {worst[2]:.3e}"


def compare(sec, name, exact, outs, refs, scales, emus, tensors):
    for got, ref, sc, emu, tn in zip(outs, refs, scales, emus, tensors):
        if exact:
            same(f"{name} {tn}", got, ref, sc)
        else:
            floaty(sec, name, tn, got, ref, sc, emu)


# ------------------------------------------------------------------------------------------------ data
class Data:
    """Integer (exact tier) or random (float tier) operands from one seeded generator."""

    def __init__(self, exact, *seed):
        self.exact, self.rng = exact, np.random.default_rng([int(exact), *seed])

    def act(self, *shape, lim=3):
        if self.exact:
            return self.rng.integers(-lim, lim + 1, shape).astype(np.float32)
        return (SCALE * self.rng.standard_normal(shape)).astype(np.float32)

    def weight(self, cout, cin, lim=2):
        if self.exact:
            return self.rng.integers(-lim, lim + 1, (cout, cin)).astype(np.float32)
        return (self.rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)

    def bias(self, n):
        return self.rng.integers(-3, 4, n).astype(np.float32) if self.exact else self.rng.standard_normal(n).astype(np.float32)

    def gate(self, n=256):
        """gateway scale, bias, PReLU slope"""
        if self.exact:
            return self.rng.choice([-2.0, -1.0, 1.0, 2.0], n).astype(np.float32), self.rng.integers(-2, 3, n).astype(np.float32), 0.5
        return (1 + 0.3 * self.rng.standard_normal(n)).astype(np.float32), self.rng.standard_normal(n).astype(np.float32), 0.25

    def caf(self, B, T, F, Tv):
        """r / att distinct per (b, tv, c); eval-BatchNorm constants (exact tier: integers, sqrt(var + eps) = 1 in float32)."""
        b, c, tv = np.meshgrid(np.arange(B), np.arange(256), np.arange(Tv), indexing="ij")
        if self.exact:
            r, att = ((5 * b + 3 * tv + c) % 5 - 2).astype(np.float32), ((3 * b + 2 * tv + 7 * c) % 4 - 1).astype(np.float32)
            var = np.full(256, 1.0 - R.EPS)  # float64 for the reference; the device gets unit_var() (caf_ptrs)
            def bn():
                return np.stack([self.rng.choice([1.0, 2.0], 256), self.rng.integers(-2, 3, 256), self.rng.integers(-2, 3, 256), var])
            wk, wv = self.rng.choice([-1.0, 1.0], 256).astype(np.float32), self.rng.choice([-1.0, 1.0], 256).astype(np.float32)
        else:
            r = (self.rng.standard_normal((B, 256, Tv)) + 0.01 * (b + tv + c)).astype(np.float32)
            att = self.rng.random((B, 256, Tv)).astype(np.float32)
            def bn():
                return np.stack([1 + 0.2 * self.rng.standard_normal(256), 0.3 * self.rng.standard_normal(256), 0.3 * self.rng.standard_normal(256),
                                 0.5 + self.rng.random(256)]).astype(np.float32)
            wk, wv = self.rng.standard_normal(256).astype(np.float32), self.rng.standard_normal(256).astype(np.float32)
        return dict(r=r, att=att, w_key=wk, bn_key=bn(), w_val=wv, bn_val=bn(), T=T, F=F, exact=self.exact)


def unit_var():
    """A float32 v with float32(v + float32(1e-5)) == 1: the kernels' sqrtf(var + eps) is then exactly 1."""
    eps, v = np.float32(1e-5), np.float32(1) - np.float32(1e-5)
    for _ in range(8):
        for cand in (v, np.nextafter(v, np.float32(2)), np.nextafter(v, np.float32(0))):
            if np.float32(cand + eps) == np.float32(1):
                return float(cand)
        v = np.nextafter(v, np.float32(2))
    raise AssertionError("no float32 variance with var + eps == 1")


def images(w):
    from rtfs_net_amd import packing
    return dv(packing.split16_image(torch.from_numpy(w)).numpy())


def proj_image(wp):
    from rtfs_net_amd import packing
    return dv(packing.split16_image(torch.from_numpy(wp)[:, torch.tensor(packing.proj_perm())]).numpy())


def taps_image(wt):
    from rtfs_net_amd import packing
    return dv(packing.taps_perm_image(torch.from_numpy(wt)).numpy())


def caf_ptrs(c, transposed=False, poison_plain=False):
    """Device arguments of a CAF description; transposed: the (B, Tv, 256) copies as well; poison_plain: the untransposed ones hold 3e38."""
    def bn(a):
        a = np.asarray(a, np.float32).copy()
        if c["exact"]:
            a[3] = unit_var()
        return dv(a)
    k = dict(caf_w_key=dv(c["w_key"]), caf_bn_key=bn(c["bn_key"]), caf_w_val=dv(c["w_val"]), caf_bn_val=bn(c["bn_val"]))
    k["caf_r"] = dv(np.full_like(c["r"], 3e38) if poison_plain else c["r"])
    k["caf_att"] = dv(np.full_like(c["att"], 3e38) if poison_plain else c["att"])
    if transposed:
        k["caf_rt"], k["caf_attt"] = dv(c["r"].transpose(0, 2, 1)), dv(c["att"].transpose(0, 2, 1))
    return k


MEMO = {}  # a case run twice (counter / static stride) computes its reference once; finish() empties it


def memo(key, fn):
    if key not in MEMO:
        MEMO[key] = fn()
    return MEMO[key]


def three(exact, fn, *a, ar=R.F16X3):
    """The op in the reference arithmetic and (float tier) in the emulation: (refs, scales, emus)."""
    refs, scales = fn(R.EXACT, *a)
    return refs, scales, ((None,) * len(refs) if exact else fn(ar, *a)[0])


def cs_options(P, padded):
    return [pitch(P), pitch(P) + 64] if padded else [0, P + 1, P + 37]


def sweep(padded, float_too=True):
    """(exact, B, P, cs) over the pixel counts, batch 1..3, every row pitch; then the float tier at a few."""
    for i, P in enumerate(PS):
        for j, cs in enumerate(cs_options(P, padded)):
            yield True, 1 + (i + j) % 3, P, cs
    if float_too:
        for i, P in enumerate(FLOAT_PS):
            yield False, 1 + i % 3, P, cs_options(P, padded)[i % len(cs_options(P, padded))]


# ------------------------------------------------------------------------------------------------ gateway + projection: pws, head4
def gateway_case(sec, op, exact, B, P, cs, x2=False, caf=None, ctr=False, seed=0):
    name = f"{sec} {'exact' if exact else 'float'} B{B} P{P} cs{cs} x2{int(x2)} caf{caf} ctr{int(ctr)}"
    COUNT[sec] = COUNT.get(sec, 0) + 1
    d = Data(exact, seed, B, P)
    x, a1 = d.act(B, 256, P), d.act(B, 256, P) if x2 else None
    gw, gb, slope = d.gate()
    wp, bp = d.weight(64, 256), d.bias(64)
    c = d.caf(B, *caf) if caf else None
    refs, scales, emus = memo(name.replace(" ctr1", " ctr0"), lambda: three(exact, R.gateway_proj, x, a1, gw, gb, slope, wp, bp, c))
    res, out = Buf(B, 256, P, cs), Buf(B, 64, P, cs)
    k = dict(x=Buf(B, 256, P, cs, x), res_out=res, out=out, w16=images(wp), bias=dv(bp), gw=dv(gw), gb=dv(gb), slope=dv([slope]))
    if x2:
        k["x2"] = Buf(B, 256, P, cs, a1)
    if c:
        k.update(caf_ptrs(c))
    if ctr:
        k["tile_ctr"] = ctr_word()
    r = call(op, B, P, cs, caf=(c["T"], c["F"], c["r"].shape[2]) if c else None, **k)
    if op == 2:
        ok(name, r, persistent(PWS, 256, 64, GATEWAY, BIAS, int(bool(c)), 0, int(x2), P, B, 256, 512, ctr))
        pad = None
    else:
        ok(name, r, persistent(HEAD4, 256, 64, GATEWAY, 0, 0, 0, 0, P, B, 256, 512, ctr))
        pad = pitch(P)
    outs = [res.take(name + " res", pad), out.take(name + " xenc", pad)]
    compare(sec, name, exact, outs, refs, scales, emus, ("residual", "x_enc"))
    return outs


CAF_SHAPES = [(1, 1), (3, 2), (5, 3), (4, 7)]  # (T, Tv): fewer and more video frames than audio frames


def test_pws_gateway_proj():
    """launch_pws_gateway_proj: plain, with x2, with x2 + the CAF prologue (reached from no API call); 256-pixel tiles (COUT 64: two pixels per lane)."""
    sec = "pws gateway"
    for exact, B, P, cs in sweep(False):
        gateway_case(sec, 2, exact, B, P, cs, x2=P % 2 == 1, ctr=P % 3 == 0)
        gateway_case(sec, 2, exact, B, P, cs, x2=P % 2 == 0, ctr=P % 3 == 1, seed=1)
    for T, Tv in CAF_SHAPES:
        for F in (43, 129):
            for exact in (True, False):
                gateway_case(sec, 2, exact, 2, T * F, [0, T * F + 37][T % 2], x2=True, caf=(T, F, Tv), ctr=bool(T % 2))
    # above the grid cap: 257 pixels = two tiles per sample, 258 samples = 516 tiles on 512 workgroups; counter and static stride agree
    a = gateway_case(sec, 2, True, 258, 257, 0, x2=True, ctr=True)
    b = gateway_case(sec, 2, True, 258, 257, 0, x2=True, ctr=False)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    finish(sec)


def test_pws_head4():
    """launch_pws_head4 (padded rows): 256-pixel tiles, whole 64-pixel wave segments, the K ring."""
    sec = "head4"
    for exact, B, P, cs in sweep(True):
        gateway_case(sec, 3, exact, B, P, cs, ctr=P % 2 == 0)
    a = gateway_case(sec, 3, True, 258, 257, 320, ctr=True)   # 516 tiles on 512 workgroups
    b = gateway_case(sec, 3, True, 258, 257, 320, ctr=False)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    finish(sec)


# ------------------------------------------------------------------------------------------------ residual conv
def residual_case(sec, exact, B, P, cs, ctr=False):
    name = f"{sec} {'exact' if exact else 'float'} B{B} P{P} cs{cs} ctr{int(ctr)}"
    COUNT[sec] = COUNT.get(sec, 0) + 1
    d = Data(exact, 2, B, P)
    x, res = d.act(B, 64, P), d.act(B, 256, P)
    w, b = d.weight(256, 64), d.bias(256)
    refs, scales, emus = memo(name.replace(" ctr1", " ctr0"), lambda: three(exact, R.residual, x, w, b, res))
    out = Buf(B, 256, P, cs)
    k = dict(x=Buf(B, 64, P, cs, x), aux=Buf(B, 256, P, cs, res), out=out, w16=images(w), bias=dv(b))
    if ctr:
        k["tile_ctr"] = ctr_word()
    ok(name, call(4, B, P, cs, **k), persistent(RES2, 64, 256, 0, BIAS_RES, 0, 0, 0, P, B, 256, 512, ctr))
    outs = [out.take(name)]
    compare(sec, name, exact, outs, refs, scales, emus, ("out",))
    return outs


def test_pws_residual():
    """launch_pws_residual -> pws_res2_kernel: two pixels per lane on rows of any pitch (odd P: a lane's pair straddles two rows)."""
    sec = "res2"
    for exact, B, P, cs in sweep(False):
        residual_case(sec, exact, B, P, cs, ctr=P % 2 == 1)
    a = residual_case(sec, True, 258, 257, 0, ctr=True)
    b = residual_case(sec, True, 258, 257, 0, ctr=False)
    assert np.array_equal(a[0], b[0])
    finish(sec)


# ------------------------------------------------------------------------------------------------ block boundary
def boundary_case(sec, op, exact, B, P, cs, am=1, caf=None, ctr=False, K=1, first=True, table=None, seed=0):
    """op 5: launch_pws_b2b, op 6: launch_pws_b2b4.  B = targets.  K > 1: K targets per mixture, `first`: x is the mixture's too (xk = K), else
    the target's own (xk = 1).  table = (mix_of, mix_base, mixtures): divisors of 0, the mixture comes from the table."""
    name = f"{sec} {'exact' if exact else 'float'} B{B} P{P} cs{cs} am{am} caf{caf} ctr{int(ctr)} K{K} first{int(first)} table{table is not None}"
    COUNT[sec] = COUNT.get(sec, 0) + 1
    d = Data(exact, 3, B, P, am, seed)
    if table:
        mix_of, mix_base, nmix = table
        of = np.asarray(mix_of) - mix_base
        xk, a1k = (0, 0) if first else (1, 0)
    else:
        nmix, of, mix_base = B // K, np.arange(B) // K, 0
        xk, a1k = (K, K) if first else (1, K)
    fan = K > 1 or table is not None
    nx = nmix if first and fan else B
    # every mixture's rows hold their own pattern: a wrong mixture index changes every element
    x = d.act(nx, 64, P) + (np.arange(nx, dtype=np.float32)[:, None, None] if exact and fan else 0)
    a1 = d.act(nmix, 256, P) + (2 * np.arange(nmix, dtype=np.float32)[:, None, None] if exact and fan else 0)
    xs, a1s = (x[of] if first and fan else x), a1[of]
    gw, gb, slope = d.gate()
    w1, b1, wp, bp = d.weight(256, 64), d.bias(256), d.weight(64, 256), d.bias(64)
    c = d.caf(B, *caf) if caf else None
    res_i = d.act(B, 256, P)
    if am & 4:   # residual_0 is not read: it is the gateway of a1 (the head kernel need not write it)
        init = None
        logical = lambda ar: R.gateway(ar, ar.t(a1s), R.t64(a1s).abs(), gw, gb, slope)[0]
    elif am & 1:
        init = res_i
        logical = lambda ar: ar.t(res_i)
    else:        # the buffer already holds residual_i + a1
        init = (res_i + a1s).astype(np.float32)
        logical = lambda ar: (R.t64(init) - R.t64(a1s)).to(ar.dtype)
    def run(ar):
        (r, y), (sr, sy) = R.boundary(ar, xs, logical(ar), a1s, w1, b1, gw, gb, slope, wp, bp, c)
        if am & 2:  # written WITH a1: the next boundary runs with bit 0 clear
            r, sr = r + ar.t(a1s), sr + R.t64(a1s).abs()
        return (r, y), (sr, sy)
    refs, scales, emus = memo(name.replace(" ctr1", " ctr0"), lambda: (*run(R.EXACT), (None, None) if exact else run(R.F16X3)[0]))
    res, xenc = Buf(B, 256, P, cs, init), Buf(B, 64, P, cs)
    # behind the mixtures lie decoy samples (other integers), as many as a target index or an un-based table entry could reach: a kernel that
    # indexes by target where it should by mixture, or forgets mix_base, reads them - inside the allocation
    def decoys(v):
        n = max(B, nmix + mix_base) - v.shape[0] if fan else 0
        return np.concatenate([v, d.act(n, *v.shape[1:]) + 50]) if n > 0 else v
    xb, a1b = decoys(x), decoys(a1)
    k = dict(x=Buf(xb.shape[0], 64, P, cs, xb), res_out=res, a1=Buf(a1b.shape[0], 256, P, cs, a1b), out=xenc, w16=images(w1), bias=dv(b1), w2_16=proj_image(wp),
             bp=dv(bp), gw=dv(gw), gb=dv(gb), slope=dv([slope]))
    if c:
        k.update(caf_ptrs(c, transposed=op == 6, poison_plain=op == 6))
    if table:
        k["mix_of"] = dv(mix_of, np.int32)
    if ctr:
        k["tile_ctr"] = ctr_word()
    cafn = (c["T"], c["F"], c["r"].shape[2]) if c else None
    if op == 5:
        assert am == 1 and K == 1 and not table and not ctr
        ok(name, call(5, B, P, cs, caf=cafn, **k), persistent(B2B, 64, 64, 0, 0, int(bool(c)), 1, 0, P, B, 512, 256, False))
        pad = None
    else:
        ok(name, call(6, B, P, cs, caf=cafn, a1_mode=am, xk=xk, a1k=a1k, mix_base=mix_base, **k),
           persistent(B2B4, 64, 64, 0, 0, int(bool(c)), am, 0, P, B, 256, 256, ctr))
        pad = pitch(P)
    outs = [res.take(name + " res", pad), xenc.take(name + " xenc", pad)]
    compare(sec, name, exact, outs, refs, scales, emus, ("residual", "x_enc"))
    return outs


def test_pws_b2b_first_generation():
    """launch_pws_b2b, both CAF forms (run by no GPU test through the API: the fused separator always qualifies for the second generation):
    512-pixel tiles, 8 waves, static stride, cap 256."""
    sec = "b2b"
    for exact, B, P, cs in sweep(False):
        boundary_case(sec, 5, exact, B, P, cs)
    for T, Tv in CAF_SHAPES:
        for F in (43, 129):
            for exact in (True, False):
                boundary_case(sec, 5, exact, 2, T * F, [0, T * F + 1][T % 2], caf=(T, F, Tv))
    boundary_case(sec, 5, True, 130, 513, 0)  # two tiles per sample, 260 tiles on 256 workgroups
    finish(sec)


@pytest.mark.parametrize("am", [0, 1, 3])
def test_pws_b2b4_plain(am):
    """launch_pws_b2b4 without a CAF, a1_mode 0 / 1 / 3: whether the residual read already contains a1, whether the written one does."""
    sec = f"b2b4 am{am}"
    for exact, B, P, cs in sweep(True):
        boundary_case(sec, 6, exact, B, P, cs, am=am, ctr=P % 2 == 0)
    for K in (2, 3):
        for first in (True, False):
            boundary_case(sec, 6, True, 2 * K, 193, 256, am=am, K=K, first=first, ctr=first)
    # 3 mixtures -> 2, 0 and 3 targets, the launch's batch part starting at mixture 5
    for first in (True, False):
        boundary_case(sec, 6, True, 5, 129, 192, am=am, first=first, table=([5, 5, 7, 7, 7], 5, 3), ctr=not first)
    a = boundary_case(sec, 6, True, 130, 257, 320, am=am, ctr=True)   # 260 tiles on 256 workgroups
    b = boundary_case(sec, 6, True, 130, 257, 320, am=am, ctr=False)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    finish(sec)


@pytest.mark.parametrize("am", [1, 3, 5, 7])
def test_pws_b2b4_caf(am):
    """launch_pws_b2b4 with the CAF between residual conv and gateway (first boundary), a1_mode 1 / 3 / 5 / 7; the kernel reads the transposed
    video tables, the untransposed ones hold 3e38."""
    sec = f"b2b4 caf am{am}"
    for T, Tv in CAF_SHAPES:
        for F in (43, 129):
            P = T * F
            for exact in (True, False):
                boundary_case(sec, 6, exact, 2, P, pitch(P) + 64 * (T % 2), am=am, caf=(T, F, Tv), ctr=bool(T % 2))
    for K in (2, 3):
        boundary_case(sec, 6, True, 2 * K, 3 * 43, 192, am=am, caf=(3, 43, 2), K=K, first=True, ctr=True)
    boundary_case(sec, 6, True, 5, 129, 192, am=am, caf=(3, 43, 2), first=True, table=([6, 6, 8, 8, 8], 6, 3))
    a = boundary_case(sec, 6, True, 130, 258, 320, am=am, caf=(2, 129, 3), ctr=True)
    b = boundary_case(sec, 6, True, 130, 258, 320, am=am, caf=(2, 129, 3), ctr=False)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    finish(sec)


# ------------------------------------------------------------------------------------------------ 256 -> 256: pwr
def bn_case(sec, op, B, P, cs=0, ctr=False, arith=R.F16X3, exact=False):
    """exact: a gLN op on integers after all - x = +-16 with as many of each per sample, so the mean is 0, the variance 256 (float32(256 + eps)
    = 256: eps is below half an ulp) and the fold's rsqrt exactly 1/16; gamma and beta integers: ReLU(x gamma / 16 + beta) and the
    1x1 conv behind it are integers.  The reference is that closed form (the float64 gLN keeps its eps)."""
    name = f"{sec} {'exact ' if exact else ''}B{B} P{P} cs{cs} ctr{int(ctr)}"
    COUNT[sec] = COUNT.get(sec, 0) + 1
    d = Data(exact, 4, B, P)
    if exact:
        sign = np.stack([d.rng.permutation(np.repeat([-1.0, 1.0], 128 * P)).reshape(256, P) for _ in range(B)]).astype(np.float32)
        x, g = 16 * sign, d.rng.integers(-3, 4, 256).astype(np.float32)
        gamma, beta = g, d.bias(256)
        w, b = d.weight(256, 256), d.bias(256)
        v = torch.relu(R.t64(sign) * R.col(g, R.EXACT) + R.col(beta, R.EXACT))
        refs, scales, emus = (R.EXACT.mm(w, v) + R.col(b, R.EXACT),), (R.absmm(w, v) + R.col(b, R.EXACT).abs(),), (None,)
    else:
        x = d.act(B, 256, P) * (1 + np.arange(B, dtype=np.float32)[:, None, None]) + 3.0  # per-sample statistics differ
        gamma, beta = (1 + 0.2 * d.rng.standard_normal(256)).astype(np.float32) * SCALE, d.bias(256) * SCALE
        w, b = d.weight(256, 256), d.bias(256)
        refs, scales = R.audio_bn(R.EXACT, x, gamma, beta, w, b)
        emus, _ = R.audio_bn(arith, x, gamma, beta, w, b)
    out = Buf(B, 256, P, cs)
    k = dict(x=Buf(B, 256, P, cs, x), out=out, bias=dv(b), stats=dv(R.stats(x).numpy(), np.float64), gamma=dv(gamma), beta=dv(beta))
    if op == 7:
        k["w16"] = images(w)
        route = persistent(PWR, 256, 256, 0, 0, 0, 0, 0, P, B, 128, 512, ctr)
    elif op == 1:
        k["w16"] = images(w)
        route = (PW16, 256, 256, GLN_RELU, BIAS, 0, 0, 0, cdiv(P, 128), cdiv(P, 128) * B, cdiv(P, 128) * B, 0)
    else:
        k["wt"] = dv(w.T)
        route = (F32K, 256, 256, GLN_RELU, BIAS, 0, 0, 0, cdiv(P, 64), cdiv(P, 64) * B, cdiv(P, 64) * B, 0)
    if ctr:
        k["tile_ctr"] = ctr_word()
    ok(name, call(op, B, P, cs, kind=0, inv_count=1.0 / (256 * P), **k), route)
    compare(sec, name, exact, [out.take(name)], refs, scales, emus, ("a1",))


def test_pwr_audio_bn():
    """launch_pwr_audio_bn: gLN fold per sample (a workgroup that walks from one sample into the next refolds), 128-pixel tiles."""
    sec = "pwr bn"
    for i, P in enumerate(PS):
        bn_case(sec, 7, 1 + i % 3, P, [0, P + 1, P + 37][i % 3], ctr=i % 2 == 0)
    for i, P in enumerate([2, 65, 129, 387]):
        bn_case(sec, 7, 1 + i % 3, P, [0, P + 37][i % 2], ctr=i % 2 == 1, exact=True)
    bn_case(sec, 7, 258, 129, 0, ctr=True)   # 516 tiles on 512 workgroups: workgroups 0..3 take a second tile, of another sample
    bn_case(sec, 7, 258, 129, 0, ctr=False)
    finish(sec)


def s3_case(sec, op, kind, exact, B, P, cs=0, ctr=False, live=18, stats=None, amp=1.0, ar=R.F16X3):
    """kind: 's3' (separated spectrum) or 'taps' (S3 + decoder taps).  stats: mean square of a0 handed to the kernel's range normalisation
    (exact tier: any power of four; float tier: True = the real statistics)."""
    name = f"{sec} {kind} {'exact' if exact else 'float'} B{B} P{P} cs{cs} ctr{int(ctr)} live{live} stats{stats} amp{amp}"
    COUNT[sec] = COUNT.get(sec, 0) + 1
    d = Data(exact, 5, B, P)
    x, a0 = d.act(B, 256, P), d.act(B, 256, P, lim=2) * np.float32(amp)
    w, b, slope = d.weight(256, 256), d.bias(256), (0.5 if exact else 0.25)
    wt = np.zeros((32, 256), np.float32)
    wt[:18] = d.weight(18, 256)
    if live > 18:  # rows 18.. of the production image are zero; a live count above 18 must write them, as zeros or as what the image holds
        wt[18:live] = d.weight(live - 18, 256)
    esc = np.ones((B, 1, 1), np.float32)
    k = dict(x=Buf(B, 256, P, cs, x), aux=Buf(B, 256, P, cs, a0), bias=dv(b), slope=dv([slope]))
    inv = 0.0
    if stats is not None:
        st = R.stats(a0).numpy() if stats is True else np.stack([np.zeros(B), np.full(B, float(stats) * 256 * P)], 1)
        k["stats"], inv = dv(st, np.float64), 1.0 / (256 * P)
        if stats is True:  # the emulation sees the operand the kernel splits: a0 times the power of two near 1 / rms(a0)
            eb = (((st[:, 1] * inv).astype(np.float32).view(np.uint32) >> 23) & 0xFF).astype(np.int64) - 127
            esc = (2.0 ** np.clip(-(eb >> 1), -40, 40)).astype(np.float32).reshape(B, 1, 1)
    if kind == "s3":
        refs, scales, emus = memo(name.replace(" ctr1", " ctr0"), lambda: three(exact, R.s3, x, slope, w, b, a0, ar=ar))
        out = Buf(B, 256, P, cs)
    else:
        refs, scales = memo(name.replace(" ctr1", " ctr0"), lambda: R.s3_taps(R.EXACT, x, slope, w, b, a0, wt, live))
        emus = [None if exact else R.s3_taps(ar, x, slope, w, b, a0 * esc, wt, live)[0][0] / torch.from_numpy(esc)]
        out = Buf(B, live, P, cs)
        k["w16b"] = taps_image(wt)
    k["out"] = out
    if ctr:
        k["tile_ctr"] = ctr_word()
    if op == 7:
        k["w16"] = images(w)
        route = persistent(PWR, 256, 256, 0, 0, 0, 0, 1 if kind == "s3" else 2, P, B, 128, 512, ctr)
        r = call(7, B, P, cs, kind=1 if kind == "s3" else 2, cout_live=live, inv_count=inv, **k)
    elif op == 1:
        k["w16"] = images(w)
        route = (PW16, 256, 256, PRELU, S3, 0, 0, 0, cdiv(P, 128), cdiv(P, 128) * B, cdiv(P, 128) * B, 0)
        r = call(1, B, P, 0, kind=3, **k)
    else:
        k["wt"] = dv(w.T)
        route = (F32K, 256, 256, PRELU, S3, 0, 0, 0, cdiv(P, 64), cdiv(P, 64) * B, cdiv(P, 64) * B, 0)
        r = call(0, B, P, 0, kind=3, **k)
    ok(name, r, route)
    outs = [out.take(name)]
    compare(sec, name, exact, outs, refs, scales, emus, (kind,))
    return outs


def test_pwr_s3():
    """launch_pwr_s3: mask rows c and c + 128 pair with the encoder rows c and c + 128 (output tiles run 0, 4, 1, 5, ...)."""
    sec = "pwr s3"
    for exact, B, P, cs in sweep(False):
        s3_case(sec, 7, "s3", exact, B, P, cs, ctr=P % 2 == 0)
    a = s3_case(sec, 7, "s3", True, 258, 129, 0, ctr=True)
    b = s3_case(sec, 7, "s3", True, 258, 129, 0, ctr=False)
    assert np.array_equal(a[0], b[0])
    finish(sec)


def test_pwr_s3_taps():
    """launch_pwr_s3_taps (PWR_S3T; the fused separator never falls back to it): the taps GEMM on accumulator-order K, 18 / 24 live rows,
    the power-of-two range normalisation cancelling exactly, a0 at the amplitudes of test_input_amplitude_range."""
    sec = "pwr s3 taps"
    for i, (exact, B, P, cs) in enumerate(sweep(False)):
        s3_case(sec, 7, "taps", exact, B, P, cs, ctr=P % 2 == 1, live=[18, 24][i % 2],
                stats=([None, 64.0, 0.25][i % 3] if exact else [None, True][i % 2]))
    for amp in (1e-5, 1e-3, 30.0, 1e4):
        s3_case(sec, 7, "taps", False, 2, 193, 0, stats=True, amp=amp)
    a = s3_case(sec, 7, "taps", True, 258, 129, 0, ctr=True, stats=64.0)
    b = s3_case(sec, 7, "taps", True, 258, 129, 0, ctr=False, stats=64.0)
    assert np.array_equal(a[0], b[0])
    finish(sec)


# ------------------------------------------------------------------------------------------------ first f16x3 generation and exact f32
def taps_case(sec, op, exact, B, P, live):
    name = f"{sec} taps {'exact' if exact else 'float'} B{B} P{P} live{live}"
    COUNT[sec] = COUNT.get(sec, 0) + 1
    d = Data(exact, 6, B, P)
    sep = d.act(B, 256, P)
    wt = np.zeros((32, 256), np.float32)
    wt[:live] = d.weight(live, 256)
    ar = R.F16X3 if op == 1 else R.F32
    refs, scales = R.taps(R.EXACT, sep, wt, live)
    emus, _ = R.taps(ar, sep, wt, live)
    out = Buf(B, live, P, 0)
    k = dict(x=Buf(B, 256, P, 0, sep), out=out)
    k["w16" if op == 1 else "wt"] = images(wt) if op == 1 else dv(wt.T)
    n = cdiv(P, 256)
    ok(name, call(op, B, P, 0, kind=4, cout_live=live, **k), (PW16 if op == 1 else F32K, 256, 32, 0, TAPS, 0, 0, 0, n, n * B, n * B, 0))
    compare(sec, name, exact, [out.take(name)], refs, scales, emus, ("z",))


def simple_cases(sec, op):
    """The five launchers of one of the two contiguous-row generations: exact integers everywhere but the gLN op, one float case each."""
    ar = R.F16X3 if op == 1 else R.F32
    fam = PW16 if op == 1 else F32K
    pts = {1: (128, 128, 64, 128, 256), 0: (64, 128, 64, 64, 256)}[op]  # pixel tile of audio_bn, gateway, residual, s3, taps
    for i, P in enumerate([1, 2, 31, 65, 129, 257, 387]):
        B = 1 + i % 3
        bn_case(sec, op, B, P, arith=ar)
        bn_case(sec, op, B, P, exact=True)
        for exact in ((True, False) if P in (65, 387) else (True,)):
            name = f"{sec} {'exact' if exact else 'float'} B{B} P{P}"
            d = Data(exact, 7, B, P)
            # gateway + projection, with and without the second addend
            x, a1 = d.act(B, 256, P), d.act(B, 256, P) if i % 2 else None
            gw, gb, slope = d.gate()
            wp, bp = d.weight(64, 256), d.bias(64)
            refs, scales = R.gateway_proj(R.EXACT, x, a1, gw, gb, slope, wp, bp)
            emus, _ = R.gateway_proj(ar, x, a1, gw, gb, slope, wp, bp)
            res, out = Buf(B, 256, P, 0), Buf(B, 64, P, 0)
            k = dict(x=Buf(B, 256, P, 0, x), res_out=res, out=out, bias=dv(bp), gw=dv(gw), gb=dv(gb), slope=dv([slope]))
            k["w16" if op == 1 else "wt"] = images(wp) if op == 1 else dv(wp.T)
            if a1 is not None:
                k["x2"] = Buf(B, 256, P, 0, a1)
            n = cdiv(P, pts[1])
            ok(name + " gateway", call(op, B, P, 0, kind=1, **k), (fam, 256, 64, GATEWAY, BIAS, 0, 0, 0, n, n * B, n * B, 0))
            compare(sec, name + " gateway", exact, [res.take(name), out.take(name)], refs, scales, emus, ("residual", "x_enc"))
            # residual conv
            ex, rs = d.act(B, 64, P), d.act(B, 256, P)
            w1, b1 = d.weight(256, 64), d.bias(256)
            refs, scales = R.residual(R.EXACT, ex, w1, b1, rs)
            emus, _ = R.residual(ar, ex, w1, b1, rs)
            out = Buf(B, 256, P, 0)
            k = dict(x=Buf(B, 64, P, 0, ex), aux=Buf(B, 256, P, 0, rs), out=out, bias=dv(b1))
            k["w16" if op == 1 else "wt"] = images(w1) if op == 1 else dv(w1.T)
            n = cdiv(P, pts[2])
            ok(name + " residual", call(op, B, P, 0, kind=2, **k), (fam, 64, 256, 0, BIAS_RES, 0, 0, 0, n, n * B, n * B, 0))
            compare(sec, name + " residual", exact, [out.take(name)], refs, scales, emus, ("out",))
            COUNT[sec] = COUNT.get(sec, 0) + 2
            s3_case(sec, op, "s3", exact, B, P, ar=ar)
            taps_case(sec, op, exact, B, P, [18, 24][i % 2])


def test_pw16_first_generation():
    """launch_pw16_*: dec_taps is the decoder's production route; audio_bn, gateway_proj, residual and s3 have no caller."""
    simple_cases("pw16", 1)
    finish("pw16")


def test_pw_exact_f32():
    """The exact-f32 A/B path (RTFS_GEMM_F32=1), launch_pw_*: held to ten times float32 torch's own error."""
    sec = "pw f32"
    simple_cases(sec, 0)
    finish(sec, "float32 torch")


# ------------------------------------------------------------------------------------------------ the fused head and tail (a0 rebuilt)
def enc_parts(d, nmix, T, F, amp=1.0):
    """Spectrogram (nmix, 2, T, F), encoder weight (256, 18) and the scratch launch_enc_stats fills.  Float tier: the weights are small, so that
    the patches the kernels split stay near SCALE once a0 is normalised to unit rms."""
    spec = d.act(nmix, 2, T, F, lim=1) * np.float32(amp)
    wenc = d.weight(256, 18, lim=1) if d.exact else (d.rng.standard_normal((256, 18)) / (SCALE * np.sqrt(18))).astype(np.float32)
    st = torch.zeros(2 * nmix + 8, dtype=torch.float64, device="cuda")
    k = dict(spec=Buf(nmix, 2, T * F, 0, spec.reshape(nmix, 2, T * F)), enc_w=dv(wenc), enc_img=torch.zeros(8192, device="cuda"),
             wpad=torch.zeros(73728, device="cuda"), stats=st)
    return spec, wenc, st, k


def check_stats(name, st, a0, nmix):
    h = host(st)
    assert (h[2 * nmix:] == 0).all(), f"{name}: statistics written past their end"
    ref = R.stats(a0).numpy()
    assert np.allclose(h[:2 * nmix].reshape(nmix, 2)[:, 1], ref[:, 1], rtol=1e-5), f"{name}: sumsq of a0"


def bn_head_case(sec, B, T, F, cs, res=True, ctr=False):
    P = T * F
    name = f"{sec} B{B} T{T} F{F} cs{cs} res{int(res)} ctr{int(ctr)}"
    COUNT[sec] = COUNT.get(sec, 0) + 1
    d = Data(False, 8, B, T, F)
    spec, wenc, st, k = enc_parts(d, B, T, F)
    gamma, beta = (1 + 0.2 * d.rng.standard_normal(256)).astype(np.float32) * SCALE, d.bias(256) * SCALE
    w, b, wp, bp = d.weight(256, 256), d.bias(256), d.weight(64, 256), d.bias(64)
    gw, gb, slope = d.gate()
    inv = 1.0 / (256 * P)
    def ref():
        refs, scales = R.bn_head(R.EXACT, spec, wenc, gamma, beta, w, b, gw, gb, slope, wp, bp)
        a0 = R.enc_a0(R.EXACT, spec, wenc)[0][0]
        emus, _ = R.bn_head(R.F16X3, spec, wenc, gamma, beta, w, b, gw, gb, slope, wp, bp, esc=R.rms_pow2(R.stats(a0).numpy(), inv))
        return refs, scales, emus, a0
    refs, scales, emus, a0 = memo(name.replace(" ctr1", " ctr0"), ref)
    a1, rs, xe = Buf(B, 256, P, cs), Buf(B, 256, P, cs) if res else None, Buf(B, 64, P, cs)
    k.update(a1=a1, res_out=rs, out=xe, w16=images(w), bias=dv(b), gamma=dv(gamma), beta=dv(beta), gw=dv(gw), gb=dv(gb), slope=dv([slope]),
             w2_16=proj_image(wp), bp=dv(bp))
    if ctr:
        k["tile_ctr"] = ctr_word()
    ok(name, call(8, B, P, cs, inv_count=inv, tf=(T, F), nmix=B, **k), persistent(BNHEAD, 256, 64, 0, 0, 0, 0, int(res), P, B, 256, 256, ctr), launches=2)
    check_stats(name, st, a0, B)
    outs = [a1.take(name + " a1", pitch(P)), rs.take(name + " res", pitch(P)) if res else None, xe.take(name + " xenc", pitch(P))]
    for i, tn in enumerate(("a1", "residual", "x_enc")):
        if outs[i] is not None:
            floaty(sec, name, tn, outs[i], refs[i], scales[i], emus[i])
    return outs


def test_bn_head():
    """launch_bn_head (k_bnh.hip) behind the production launch_enc_stats: a0 rebuilt from the spectrogram (top and bottom rows of the 3x3 conv
    at T = 1 .. 5, the frequency wrap at F = 129 and 43), one- to three-tile samples, `res` written and not, counter and static stride."""
    sec = "bn_head"
    for i, T in enumerate([1, 2, 3, 4, 5]):
        for j, cs in enumerate([pitch(T * 129), pitch(T * 129) + 64]):
            bn_head_case(sec, 1 + (i + j) % 3, T, 129, cs, res=bool((i + j) % 2), ctr=bool(j))
    bn_head_case(sec, 2, 3, 43, 192, res=True, ctr=True)
    bn_head_case(sec, 2, 5, 13, 128, res=False)  # P = 65: one live pixel in the second wave segment
    a = bn_head_case(sec, 130, 2, 129, 320, res=True, ctr=True)   # 260 tiles on 256 workgroups
    b = bn_head_case(sec, 130, 2, 129, 320, res=True, ctr=False)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    finish(sec)


def tail_case(sec, exact, B, T, F, cs, K=1, table=None, live=18, stats=True, ctr=False, amp=1.0):
    """B targets.  K > 1: target t reads the spectrogram and statistics of mixture t / K; table = (mix_of, mix_base, mixtures): K = 0."""
    P = T * F
    name = f"{sec} {'exact' if exact else 'float'} B{B} T{T} F{F} cs{cs} K{K} table{table is not None} live{live} stats{int(stats)} ctr{int(ctr)} amp{amp}"
    COUNT[sec] = COUNT.get(sec, 0) + 1
    d = Data(exact, 9, B, T, F, K)
    if table:
        mix_of, mix_base, nmix = table
        of, Karg = np.asarray(mix_of) - mix_base, 0
    else:
        nmix, of, mix_base, Karg = B // K, np.arange(B) // K, 0, K
    ntot = max(B, nmix + mix_base) if (K > 1 or table) else nmix  # decoy mixtures behind the real ones (see boundary_case)
    spec, wenc, st, k = enc_parts(d, ntot, T, F, amp)
    lim = 1 if exact else 2
    x, res = d.act(B, 64, P, lim=1), d.act(B, 256, P, lim=1)
    w1, b1, w, b, slope = d.weight(256, 64, lim), d.bias(256), d.weight(256, 256, lim), d.bias(256), (0.5 if exact else 0.25)
    wt = np.zeros((32, 256), np.float32)
    wt[:live] = d.weight(live, 256, lim)
    inv = 1.0 / (256 * P)
    def ref():
        refs, scales = R.tail(R.EXACT, x, res, spec, wenc, w1, b1, slope, w, b, wt, live, mix=of)
        a0 = R.enc_a0(R.EXACT, spec, wenc)[0][0]
        esc = R.rms_pow2(R.stats(a0).numpy(), inv) if stats else None
        emus = (None,) if exact else R.tail(R.F16X3, x, res, spec, wenc, w1, b1, slope, w, b, wt, live, mix=of, esc=esc)[0]
        return refs, scales, emus, a0
    refs, scales, emus, a0 = memo(name.replace(" ctr1", " ctr0"), ref)
    xb, rb, z = Buf(B, 64, P, cs, x), Buf(B, 256, P, cs, res), Buf(B, live, P, cs)
    k.update(x=xb, res_out=rb, out=z, w2_16=images(w1), bp=dv(b1), w16=images(w), bias=dv(b), slope=dv([slope]), w16b=taps_image(wt))
    if table:
        k["mix_of"] = dv(mix_of, np.int32)
    if ctr:
        k["tile_ctr"] = ctr_word()
    ok(name, call(9, B, P, cs, kind=0 if stats else 1, cout_live=live, inv_count=inv, xk=Karg, mix_base=mix_base, tf=(T, F), nmix=ntot, **k),
       persistent(TAIL, 64, 256, 0, 0, 0, 0, Karg, P, B, 256, 256, ctr), launches=2)
    check_stats(name, st, a0, ntot)
    xb.untouched(name + " x")
    rb.untouched(name + " res")
    outs = [z.take(name, pitch(P))]
    compare(sec, name, exact, outs, refs, scales, emus, ("z",))
    return outs


def test_tail_s3t():
    """launch_tail_s3t (k_s3f.hip) behind the production launch_enc_stats: residual conv, mask, complex product with the rebuilt a0 (rows c and
    c + 128), taps with 18 / 24 live rows, the range normalisation on and off, K targets per mixture and the table form, a0 at the amplitudes
    of test_input_amplitude_range."""
    sec = "tail"
    for i, T in enumerate([1, 2, 3, 4, 5]):
        for j, cs in enumerate([pitch(T * 129), pitch(T * 129) + 64]):
            for exact in (True, False):
                tail_case(sec, exact, 1 + (i + j) % 3, T, 129, cs, live=[18, 24][(i + j) % 2], stats=bool((i + j + exact) % 2), ctr=bool(j))
    tail_case(sec, True, 2, 3, 43, 192, ctr=True)
    tail_case(sec, True, 2, 5, 13, 128)
    for K in (2, 3):
        tail_case(sec, True, 2 * K, 2, 129, 320, K=K, ctr=K == 2)
    tail_case(sec, True, 5, 1, 129, 192, table=([5, 5, 7, 7, 7], 5, 3))
    tail_case(sec, False, 5, 2, 129, 320, table=([5, 5, 7, 7, 7], 5, 3), ctr=True)
    for amp in (1e-5, 1e-3, 30.0, 1e4):
        tail_case(sec, False, 2, 2, 129, 320, amp=amp)
    a = tail_case(sec, True, 130, 2, 129, 320, ctr=True)   # 260 tiles on 256 workgroups
    b = tail_case(sec, True, 130, 2, 129, 320, ctr=False)
    assert np.array_equal(a[0], b[0])
    finish(sec)


def test_fused_refusals():
    """launch_bn_head / launch_tail_s3t refuse with RTFS_ERR_ARG (the caller falls back): T F != P, P < 64, a pitch that is 0, not a multiple
    of 64 or below pitch(P), and (the tail alone: its taps accumulator has 24 rows' worth of stores) cout_live > 24.  The entry has run
    launch_enc_stats by then: one launch, no route, no output written."""
    d = Data(True, 10)
    B = 2
    def head(T, F, P, cs):
        spec, wenc, st, k = enc_parts(d, B, T, F)
        big = max(cs, pitch(P))
        a1, xe = Buf(B, 256, P, big), Buf(B, 64, P, big)
        gw, gb, slope = d.gate()
        k.update(a1=a1, out=xe, w16=images(d.weight(256, 256)), bias=dv(d.bias(256)), gamma=dv(d.bias(256)), beta=dv(d.bias(256)), gw=dv(gw),
                 gb=dv(gb), slope=dv([slope]), w2_16=proj_image(d.weight(64, 256)), bp=dv(d.bias(64)))
        return call(8, B, P, cs, inv_count=1.0 / (256 * P), tf=(T, F), nmix=B, **k), (a1, xe)
    def tail(T, F, P, cs, live=18):
        spec, wenc, st, k = enc_parts(d, B, T, F)
        big = max(cs, pitch(P))
        z = Buf(B, live, P, big)
        k.update(x=Buf(B, 64, P, big, d.act(B, 64, P)), res_out=Buf(B, 256, P, big, d.act(B, 256, P)), out=z, w2_16=images(d.weight(256, 64)),
                 bp=dv(d.bias(256)), w16=images(d.weight(256, 256)), bias=dv(d.bias(256)), slope=dv([0.5]), w16b=taps_image(np.zeros((32, 256), np.float32)))
        return call(9, B, P, cs, cout_live=live, inv_count=1.0 / (256 * P), tf=(T, F), nmix=B, **k), (z,)
    for what, fn in (("bn_head", head), ("tail", tail)):
        for why, a in (("T F != P", (2, 129, 257, 320)), ("P < 64", (1, 43, 43, 64)), ("cs 0", (1, 129, 129, 0)), ("cs % 64", (1, 129, 129, 224)),
                       ("cs < pitch", (1, 129, 129, 128))):
            r, outs = fn(*a)
            refused(f"{what} {why}", r, ERR_ARG, *outs, launches=1)
    r, outs = tail(1, 129, 129, 192, live=25)
    refused("tail cout_live 25", r, ERR_ARG, *outs, launches=1)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    """Every condition the launchers refuse on: status as documented, nothing launched, the route record empty, nothing written."""
    d = Data(True, 9)
    B, P = 2, 100
    cs = pitch(P)
    gw, gb, slope = d.gate()
    wp, bp, w1, b1 = d.weight(64, 256), d.bias(64), d.weight(256, 64), d.bias(256)
    c = d.caf(B, 4, 25, 3)
    def gk(cs_, x2=False, P_=P):
        res, out = Buf(B, 256, P_, cs_ if cs_ >= P_ else P_), Buf(B, 64, P_, cs_ if cs_ >= P_ else P_)
        k = dict(x=Buf(B, 256, P_, max(cs_, P_), d.act(B, 256, P_)), res_out=res, out=out, w16=images(wp), bias=dv(bp), gw=dv(gw), gb=dv(gb),
                 slope=dv([slope]))
        if x2:
            k["x2"] = Buf(B, 256, P_, max(cs_, P_), d.act(B, 256, P_))
        return k, (res, out)
    # streaming gateway + projection
    k, o = gk(0); refused("pws caf without x2", call(2, B, P, 0, caf=(4, 25, 3), **k, **caf_ptrs(c)), ERR_ARG, *o)
    k, o = gk(0, P_=1); refused("pws P 1", call(2, B, 1, 0, **k), ERR_SHAPE, *o)
    k, o = gk(P - 1); refused("pws cs < P", call(2, B, P, P - 1, **k), ERR_SHAPE, *o)
    # head on padded rows
    k, o = gk(cs, x2=True); refused("head4 x2", call(3, B, P, cs, **k), ERR_ARG, *o)
    k, o = gk(0); refused("head4 cs 0", call(3, B, P, 0, **k), ERR_ARG, *o)
    k, o = gk(cs + 32); refused("head4 cs % 64", call(3, B, P, cs + 32, **k), ERR_ARG, *o)
    k, o = gk(64); refused("head4 cs < pitch", call(3, B, P, 64, **k), ERR_ARG, *o)
    k, o = gk(64, P_=1); refused("head4 P 1", call(3, B, 1, 64, **k), ERR_ARG, *o)
    k, o = gk(cs); refused("head4 caf", call(3, B, P, cs, caf=(4, 25, 3), **k, **caf_ptrs(c)), ERR_ARG, *o)
    # residual conv
    def rk(cs_, P_=P):
        out = Buf(B, 256, P_, max(cs_, P_))
        return dict(x=Buf(B, 64, P_, max(cs_, P_), d.act(B, 64, P_)), aux=Buf(B, 256, P_, max(cs_, P_), d.act(B, 256, P_)), out=out, w16=images(w1),
                    bias=dv(b1)), out
    k, o = rk(P - 1); refused("res2 cs < P", call(4, B, P, P - 1, **k), ERR_SHAPE, o)
    k, o = rk(0, 1); refused("res2 P 1", call(4, B, 1, 0, **k), ERR_SHAPE, o)
    # block boundaries
    def bk(cs_, caf_=False, transposed=True, P_=P):
        big = max(cs_, pitch(P_))
        res, xenc = Buf(B, 256, P_, big, d.act(B, 256, P_)), Buf(B, 64, P_, big)
        k = dict(x=Buf(B, 64, P_, big, d.act(B, 64, P_)), res_out=res, a1=Buf(B, 256, P_, big, d.act(B, 256, P_)), out=xenc, w16=images(w1),
                 bias=dv(b1), w2_16=proj_image(wp), bp=dv(bp), gw=dv(gw), gb=dv(gb), slope=dv([slope]))
        if caf_:
            k.update(caf_ptrs(c, transposed=transposed))
        return k, (res, xenc)
    k, o = bk(P - 1); refused("b2b cs < P", call(5, B, P, P - 1, **k), ERR_SHAPE, *o)
    k, o = bk(0, P_=1); refused("b2b P 1", call(5, B, 1, 0, **k), ERR_SHAPE, *o)
    k, o = bk(0); refused("b2b4 cs 0", call(6, B, P, 0, **k), ERR_ARG, *o)
    k, o = bk(cs + 32); refused("b2b4 cs % 64", call(6, B, P, cs + 32, **k), ERR_ARG, *o)
    k, o = bk(64); refused("b2b4 cs < pitch", call(6, B, P, 64, **k), ERR_ARG, *o)
    k, o = bk(64, P_=1); refused("b2b4 P 1", call(6, B, 1, 64, **k), ERR_ARG, *o)
    for am in (2, 4, 6, 5, 7, 8, -1):  # 5 / 7: bit 2 without a CAF
        k, o = bk(cs); refused(f"b2b4 a1_mode {am}", call(6, B, P, cs, a1_mode=am, **k), ERR_ARG, *o)
    for am in (0, 2, 4, 6):            # a CAF needs bit 0: the first boundary's residual never contains a1
        k, o = bk(cs, caf_=True); refused(f"b2b4 caf a1_mode {am}", call(6, B, P, cs, caf=(4, 25, 3), a1_mode=am, **k), ERR_ARG, *o)
    k, o = bk(cs, caf_=True, transposed=False); refused("b2b4 caf without the transposed tables", call(6, B, P, cs, caf=(4, 25, 3), **k), ERR_ARG, *o)
    # 256 -> 256
    out = Buf(B, 256, P, P)
    k = dict(x=Buf(B, 256, P, P, d.act(B, 256, P)), aux=Buf(B, 256, P, P, d.act(B, 256, P)), out=out, w16=images(d.weight(256, 256)),
             bias=dv(d.bias(256)), slope=dv([0.5]))
    refused("pwr cs < P", call(7, B, P, P - 1, kind=1, **k), ERR_SHAPE, out)
    refused("pwr taps without the taps image", call(7, B, P, 0, kind=2, cout_live=18, **k), ERR_ARG, out)
    # the entry point itself
    refused("unknown op 10", call(10, B, P, 0, **k), ERR_ARG, out)
    refused("unknown op -1", call(-1, B, P, 0, **k), ERR_ARG, out)
    refused("fused head without its T, F and images", call(8, B, P, 0, **k), ERR_ARG, out)
    refused("unknown kind", call(7, B, P, 0, kind=3, **k), ERR_ARG, out)
    refused("pw16 with a pitch", call(1, B, P, P + 1, kind=3, **k), ERR_ARG, out)
    refused("B 0", call(7, 0, P, 0, kind=1, **k), ERR_ARG, out)
