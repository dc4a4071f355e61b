"""The two-pass route of the RTFS block's steps 15-17 (csrc/k_dw.hip dw2p_body, api.hip block_body): "15 + 16" rebuilds xf0 from c0 and only
accumulates the statistics of the concat layer's local conv, "15 + 17" rebuilds it again and writes `expanded`; xf0 is not written.

1. Kernel level, through rtfs_debug_dw_f32 ops 6 and 7, on the same inputs as today's three launches (op 0 three times):
   * S_L2 and `expanded` against the float64 restatement in tests/dw_reference.py, at the bars tests/test_hip_dw_edges.py applies
     (stats_close; floaty: ten times the error of the same formula in float32 torch, below 1e-4), every consumer fed its producer's
     float64 statistics;
   * against the three-launch result.  Both are float32 evaluations of one formula in a different order (packed FMA chains there, plain
     FMA chains on scalar weights here; another summation order of the statistics), so they may differ by what either differs from float64:
     `expanded` at the section's float bar, the statistics at twice stats_close's bars (each side meets them once);
   * outputs and the xf0 buffer are poisoned (NaN, or the poisoned run's pattern) before every call: the guard behind `expanded`, the padding
     behind every channel plane and the whole xf0 buffer must come back untouched.
   Shapes: W = 129, C in {4, 64}, B in {1, 3}, H over the band edges of both passes (1 .. 5, 23 .. 25, 47 .. 49, 64, 65; 251 once), Hg =
   max(H // 2, 1), Wg = 64, padded and unpadded channel stride, both walk directions, requested band heights 8 / 24 / 64; and every band
   height band_rows() can hand out (8, 16, .. 64) at C = 256, B = 4, H = TH + 3, where 512 workgroups keep the requested height.
2. Refusals (W != 129, C % 4 != 0, a gather geometry the row route rejects): RTFS_ERR_ARG, no launch, no route, nothing written.
3. Model level: RTFS-Net-4 forwards with rtfs_set_dw_two_pass(2) against the CPU oracle (1e-4 max-rel, 1e-5 l2-rel) and against the same
   forward with the setter at 1 (same bars: two float32 routes of one formula), and the launch counts of the three settings."""
import numpy as np
import pytest
import torch

from oracle import rtfs_oracle as O
from oracle.params import make_inputs
from tests import dw_reference as D
from tests import test_hip_dw_edges as E
from tests.test_hip_parity import SD, _conf, close, dev, host
from tests.util import rel_err

pytestmark = pytest.mark.gpu

W, WG = 129, 64
P2 = 9  # route family of the two-pass launcher (include/rtfs_amd.h)
HS = [1, 2, 3, 4, 5, 23, 24, 25, 47, 48, 49, 64, 65]


def _lib():
    return E._L()


def _poisoned(t, n, name):
    """A buffer of n floats nobody may write: still NaN, or still the poisoned run's byte pattern, and the guard behind it whole."""
    h = E._take(t, n, name)
    _, L = _lib()
    if L._POISON is None:
        assert np.isnan(h).all(), f"{name}: written"
    else:
        assert (h.view(np.uint8) == L._POISON).all(), f"{name}: written"


def _padding_untouched(flat, B, C, H, cs, name):
    """The floats behind every channel plane (cs > H W) are nobody's to write."""
    if cs == H * W:
        return
    pad = flat.reshape(B, C, cs)[:, :, H * W:]
    _, L = _lib()
    if L._POISON is None:
        assert np.isnan(pad).all(), f"{name}: channel padding written"
    else:
        assert (np.ascontiguousarray(pad).view(np.uint8) == L._POISON).all(), f"{name}: channel padding written"


class Case:
    """One set of inputs of steps 15-17 with its float64 reference and float32 restatement (computed once, shared by every launch)."""

    def __init__(self, B, C, H, cs, seed=0):
        self.B, self.C, self.H, self.cs = B, C, H, cs
        Hg = self.Hg = max(H // 2, 1)
        rng = np.random.default_rng([seed, B, C, H, cs])
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        self.keep = []
        c0 = f(B, C, H, W)
        w0, w1 = (0.3 * f(C, 16)).astype(np.float32), (0.3 * f(C, 16)).astype(np.float32)
        G0, E0, G2, E2 = f(B, C, Hg, WG), f(B, C, Hg, WG), f(B, C, Hg, WG), f(B, C, Hg, WG)
        gb = {n: E._gb(rng, C) for n in ("c0", "l0", "g0", "e0", "l2", "g2", "e2")}
        c0st = D.stats(D.t64(c0))
        gst = {n: D.stats(D.t64(v)) for n, v in (("g0", G0), ("e0", E0), ("g2", G2), ("e2", E2))}

        def chain(dt, l0st=None, l2st=None):
            t = lambda a: torch.as_tensor(a).to(dt)
            d0 = D.fold(t(c0), c0st, *gb["c0"])
            l0 = D.conv_s1(d0, w0)
            l0st = D.stats(l0) if l0st is None else l0st
            xf0 = D.apply(d0, w0, l0st, gb["l0"], t(G0), gst["g0"], gb["g0"], t(E0), gst["e0"], gb["e0"])
            l2 = D.conv_s1(xf0, w1)
            l2st = D.stats(l2) if l2st is None else l2st
            exp = D.apply(xf0, w1, l2st, gb["l2"], t(G2), gst["g2"], gb["g2"], t(E2), gst["e2"], gb["e2"], t(c0), c0st, gb["c0"])
            return l0st, l2, l2st, exp
        self.l0st, self.l2_64, self.l2st, self.exp64 = chain(torch.float64)
        _, _, _, self.exp32 = chain(torch.float32, self.l0st, self.l2st)  # (a consumer's comparison does not inherit its producer's error)
        d = self.d
        icF, icG = 1.0 / (C * H * W), 1.0 / (C * Hg * WG)
        geo = dict(B=B, C=C, H=H, W=W, Hg=Hg, Wg=WG, cs=cs)
        x = E.strided(c0, cs)
        fold0 = dict(in_stats=d(c0st.numpy(), np.float64), in_gamma=d(gb["c0"][0]), in_beta=d(gb["c0"][1]), in_inv=icF)
        # step 15's description: the first layer (its out[0] is the xf0 buffer - the new ops must leave it alone)
        self.first = dict(geo, x=x, **fold0, w=[d(w0)], in_affine=True, mode=2, loc_stats=d(self.l0st.numpy(), np.float64), loc_inv=icF,
                          loc_gamma=d(gb["l0"][0]), loc_beta=d(gb["l0"][1]), gate=d(G0), gate_stats=d(gst["g0"].numpy(), np.float64),
                          gate_gamma=d(gb["g0"][0]), gate_beta=d(gb["g0"][1]), emb=d(E0), emb_stats=d(gst["e0"].numpy(), np.float64),
                          emb_gamma=d(gb["e0"][0]), emb_beta=d(gb["e0"][1]), g_inv=icG)
        # step 16's and 17's: the second layer (17 reads the float64 statistics of conv(xf0))
        self.stat = dict(geo, w=[d(w1)], mode=1)
        self.apply = dict(geo, w=[d(w1)], mode=2, loc_stats=d(self.l2st.numpy(), np.float64), loc_inv=icF, loc_gamma=d(gb["l2"][0]),
                          loc_beta=d(gb["l2"][1]), gate=d(G2), gate_stats=d(gst["g2"].numpy(), np.float64), gate_gamma=d(gb["g2"][0]),
                          gate_beta=d(gb["g2"][1]), emb=d(E2), emb_stats=d(gst["e2"].numpy(), np.float64), emb_gamma=d(gb["e2"][0]),
                          emb_beta=d(gb["e2"][1]), g_inv=icG, addend=x, add_stats=fold0["in_stats"], add_gamma=fold0["in_gamma"],
                          add_beta=fold0["in_beta"], add_inv=icF)
        self.old = None

    def d(self, a, dtype=np.float32):
        self.keep.append(E.dv(a, dtype))
        return self.keep[-1]

    @property
    def n(self):
        return self.B * self.C * self.cs

    def name(self, what, TH, rev):
        return f"{what} B{self.B} C{self.C} H{self.H} cs{self.cs} TH{TH} rev{rev}"

    def three_launches(self):
        """Today's ops: 15 writes xf0, 16 reads it for the statistics, 17 reads it beside c0 (fed the float64 statistics, as the new op)."""
        if self.old is None:
            B, name = self.B, self.name("three launches", 0, 0)
            xf0, out, st = E._out(self.n), E._out(self.n), E._stats_buf(B)
            rc, n, _ = E.call(0, E.desc(**dict(self.first, out=[xf0], TH=24)))
            assert rc == 0 and n == 1, (name, rc, n)
            rc, n, _ = E.call(0, E.desc(**dict(self.stat, x=xf0, stats_out=[st], TH=64, rev=1)))
            assert rc == 0 and n == 1, (name, rc, n)
            rc, n, _ = E.call(0, E.desc(**dict(self.apply, x=xf0, out=[out], TH=24, rev=1)))
            assert rc == 0 and n == 1, (name, rc, n)
            self.old = (E.unstrided(E._take(out, self.n, name), B, self.C, self.H, W, self.cs), E._take_stats(st, B, name))
        return self.old

    def two_pass(self, sec, TH, rev, eff=None):
        """Ops 6 and 7 on poisoned buffers; everything compared, the route asserted.  eff: the effective band heights (pass A, pass B)."""
        B, C, H = self.B, self.C, self.H
        gx = C // 4
        thA, thB = eff or (E.band_rows(TH, H, gx, B, 320), E.band_rows(TH, H, gx, B, 768))
        E.COUNT[sec] = E.COUNT.get(sec, 0) + 1
        xf0, out, st = E._out(self.n), E._out(self.n), E._stats_buf(B)
        first = E.desc(**dict(self.first, out=[xf0], TH=24))
        name = self.name("pass A", TH, rev)
        rc, n, route = E.call(6, first, E.desc(**dict(self.stat, x=xf0, stats_out=[st], TH=TH, rev=rev)))
        assert rc == 0 and n == 1, f"{name}: status {rc}, {n} launches"
        assert route == [(P2, 2, 1, 1, 10, thA, gx, E.cdiv(H, thA))], f"{name}: route {route}"
        got_st = E._take_stats(st, B, name)
        E.stats_close(name, got_st, self.l2_64)
        _poisoned(xf0, self.n, f"{name}: xf0")
        _poisoned(out, self.n, f"{name}: expanded")
        name = self.name("pass B", TH, rev)
        rc, n, route = E.call(7, first, E.desc(**dict(self.apply, x=xf0, out=[out], TH=TH, rev=rev)))
        assert rc == 0 and n == 1, f"{name}: status {rc}, {n} launches"
        assert route == [(P2, 2, 1, 2, 11, thB, gx, E.cdiv(H, thB))], f"{name}: route {route}"
        flat = E._take(out, self.n, name)
        _padding_untouched(flat, B, C, H, self.cs, name)
        _poisoned(xf0, self.n, f"{name}: xf0")
        assert np.array_equal(E._take_stats(st, B, name), got_st), f"{name}: statistics written by the apply pass"
        got = E.unstrided(flat, B, C, H, W, self.cs)
        E.floaty(sec, name, "expanded", got, self.exp64.numpy(), self.exp32.numpy())
        old, old_st = self.three_launches()
        E.FLOAT.setdefault(sec + " vs three launches", []).append((name, "expanded", rel_err(got, old), rel_err(self.exp32.numpy(), self.exp64.numpy())))
        f = self.l2_64.reshape(B, -1)
        d0, b0 = np.abs(got_st[:, 0] - old_st[:, 0]), 2e-5 * f.abs().sum(1).numpy()
        assert (d0 <= b0).all(), f"{name}: sum differs from the three-launch route by {d0.max():.3e} (bar {b0.min():.3e})"
        d1 = np.abs(got_st[:, 1] - old_st[:, 1]) / old_st[:, 1]
        assert (d1 <= 2e-5).all(), f"{name}: sumsq differs from the three-launch route by {d1.max():.3e} rel"


def _finish(sec):
    """The section's bar from its float32 restatements (E.finish); the comparison with the three-launch route is held to the same bar."""
    rows = E.FLOAT.get(sec, [])
    bar = 10 * max(r[3] for r in rows)
    vs = E.FLOAT.pop(sec + " vs three launches", [])
    E.finish(sec)
    worst = max(vs, key=lambda r: r[2])
    print(f"[dw two-pass] {sec}: against the three-launch route worst {worst[2]:.3e} ({worst[0]}), bar {bar:.3e}")
    bad = [r for r in vs if not r[2] <= bar]
    assert not bad, f"{sec}: {len(bad)} of {len(vs)} tensors differ from the three-launch route by more than {bar:.3e}, worst {worst[0]}: {worst[2]:.3e}"


# ------------------------------------------------------------------------------------------------ 1. kernel level
@pytest.mark.parametrize("C,B", [(4, 1), (4, 3), (64, 1), (64, 3)])
def test_two_pass_band_edges(C, B):
    sec = f"two-pass C{C} B{B}"
    for H in HS + ([251] if (C, B) == (4, 1) else []):
        for cs in (H * W, E.pitch(H * W)):
            case = Case(B, C, H, cs)
            for TH in (8, 24, 64):
                for rev in (0, 1):
                    case.two_pass(sec, TH, rev)
    _finish(sec)


def test_two_pass_every_band_height():
    """512 workgroups keep the requested height: C = 256 (gx = 64), B = 4, two bands - the second of three rows."""
    sec = "two-pass band heights"
    for k, TH in enumerate(range(8, 72, 8)):
        H = TH + 3
        case = Case(4, 256, H, E.pitch(H * W), seed=1)
        case.two_pass(sec, TH, k & 1, eff=(TH, TH))
    _finish(sec)


# ------------------------------------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize("what", ["W128", "C6", "Wg65", "Hg14"])
def test_two_pass_refusals(what):
    """A shape the launcher does not take: RTFS_ERR_ARG, no launch, no route, nothing written.  W = 128: not the row mapping's width; C = 6:
    a workgroup is four channel rows; Wg = 65: 2 Wg > W, a pair's two source columns are not shared with the next lane; Hg = 14 for H = 46:
    floor(t Hg / H) is not torch's float32 nearest index there (tests/nearest_cases.py)."""
    from tests.nearest_cases import departs
    B, C, H = 2, 4, 46
    assert departs(14, 46)
    case = Case(B, C, H, H * W)
    geo = {"W128": dict(W=128), "C6": dict(C=6), "Wg65": dict(Wg=65), "Hg14": dict(Hg=14)}[what]
    xf0, out, st = E._out(case.n), E._out(case.n), E._stats_buf(B)
    first = E.desc(**dict(case.first, out=[xf0], TH=24, **geo))
    for op, second in ((6, dict(case.stat, x=xf0, stats_out=[st], TH=64, **geo)), (7, dict(case.apply, x=xf0, out=[out], TH=24, **geo))):
        rc, n, route = E.call(op, first, E.desc(**second))
        assert rc == E.ERR_ARG and n == 0 and route == [], f"{what} op {op}: status {rc}, {n} launches, route {route}"
    E._untouched(out, case.n, f"{what}: expanded")
    E._untouched(xf0, case.n, f"{what}: xf0")
    assert not E._take_stats(st, B, what).any(), f"{what}: statistics written by a refused call"


# ------------------------------------------------------------------------------------------------ 3. model level
_MODEL = []


def model():
    """This file's own RTFS-Net-4: an inference forward leaves its side stream on the model object, and other files deep-copy the model
    they share (tests/test_hip_parity.py model()) for their training steps."""
    import rtfs_net_amd as R
    if not _MODEL:
        m = R.AVNet(print_macs=False, **_conf(4))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in SD.items()})
        _MODEL.append(m.cuda().eval())
    return _MODEL[0]


def _forward(mode, wav, emb):
    """-> (output, library launches of the second of two forwards) with rtfs_set_dw_two_pass(mode); the setting is put back to 0."""
    lib, _ = _lib()
    m = model()
    try:
        assert lib.rtfs_set_dw_two_pass(mode) == 0
        with torch.no_grad():
            m(dev(wav), dev(emb))
            torch.cuda.synchronize()
            n0 = lib.rtfs_debug_launch_count()
            y = host(m(dev(wav), dev(emb)))
            return y, lib.rtfs_debug_launch_count() - n0
    finally:
        assert lib.rtfs_set_dw_two_pass(0) == 0


@pytest.mark.parametrize("B,L,Tv", [(2, 4096, 7), (1, 32000, 50)])
def test_two_pass_forward(B, L, Tv):
    wav, emb = make_inputs(B, L, Tv, 1500 + B)
    ref = O.avnet_forward(wav, emb, SD, repeats=4)
    two, n2 = _forward(2, wav, emb)
    three, n3 = _forward(1, wav, emb)
    auto, n0 = _forward(0, wav, emb)
    print(f"[dw two-pass] B{B} L{L}: launches per forward: two-pass {n2}, three launches {n3}, by size {n0}")
    close(f"two-pass forward B{B} L{L} vs oracle", two, ref)
    close(f"three-launch forward B{B} L{L} vs oracle", three, ref)
    close(f"two-pass forward B{B} L{L} vs three launches", two, three)
    assert n2 == n3 - 4, f"forced two-pass {n2} launches, forced three-launch {n3}: four blocks, one launch fewer each"
    assert n0 == n3, f"by size: {n0} launches at B = {B}, three-launch route {n3}"
    assert np.array_equal(auto, three), "by size, a small batch must take today's three launches"


def test_two_pass_setter_range():
    lib, _ = _lib()
    try:
        assert lib.rtfs_set_dw_two_pass(3) == E.ERR_ARG and lib.rtfs_set_dw_two_pass(-1) == E.ERR_ARG
        assert all(lib.rtfs_set_dw_two_pass(k) == 0 for k in (1, 2, 0))
    finally:
        lib.rtfs_set_dw_two_pass(0)
