"""CPU: ties tests/pw_reference.py (the float64 restatement tests/test_hip_pw_edges.py holds the pointwise kernels to) to
oracle/rtfs_oracle.py, which tests/test_oracle_golden.py pins against the reference project's own vectors.  Bar: the 2e-5 of
tests/test_dw_reference_host.py.  Also: the two non-reference arithmetics of that file stay near the reference, and the error measure
behaves."""
import numpy as np
import torch

from oracle import rtfs_oracle as O
from oracle.params import make_state_dict
from tests import pw_reference as R
from tests.util import rand, rel_err, spec_R4

TOL = 2e-5
SD = make_state_dict(spec_R4(), 0)
BLK = O._sub(SD, "refinement_module.audio_net.blocks")
CAF = O._sub(SD, "refinement_module.crossmodal_fusion.fusion_module.audio_lstm")
T, F = 3, 129
P = T * F


def _w(p, name):
    q = O._sub(p, name)
    w = q["full_layer.2.weight"]
    return w.reshape(w.shape[0], -1), q.get("full_layer.2.bias")


def _gate(p):
    gw, gb = _w(p, "gateway")
    return gw.reshape(-1), gb, float(np.asarray(p["gateway.full_layer.4.weight"]).reshape(-1)[0])


def _flat(x):
    return x.reshape(x.shape[0], x.shape[1], -1)


def _caf_args(video, T_):
    r, att = O.caf_video_terms(video, CAF)
    def bn(n):
        q = n + ".full_layer.3."
        return np.stack([CAF[q + "weight"], CAF[q + "bias"], CAF[q + "running_mean"], CAF[q + "running_var"]])
    return dict(r=r, att=att, w_key=CAF["key_embed.full_layer.2.weight"].reshape(-1), bn_key=bn("key_embed"),
                w_val=CAF["value_embed.full_layer.2.weight"].reshape(-1), bn_val=bn("value_embed"), T=T_, F=F)


def test_audio_bn_is_the_bottleneck():
    a0 = rand((2, 256, T, F), 11)
    p = O._sub(SD, "audio_bottleneck")
    w, b = p["full_layer.2.weight"].reshape(256, 256), p["full_layer.2.bias"]
    (y,), _ = R.audio_bn(R.EXACT, _flat(a0), p["full_layer.0.norm.weight"], p["full_layer.0.norm.bias"], w, b)
    e = rel_err(y.numpy().reshape(a0.shape), O.conv_norm_act(a0, p, pre_norm="gLN", pre_act="ReLU"))
    assert e <= TOL, e


def test_gateway_projection_and_residual_are_the_block_pieces():
    x = rand((2, 256, T, F), 12)
    gw, gb, slope = _gate(BLK)
    wp, bp = _w(BLK, "projection")
    (r, y), _ = R.gateway_proj(R.EXACT, _flat(x), None, gw, gb, slope, wp, bp)
    res = O.conv_norm_act(x, O._sub(BLK, "gateway"), groups=256, act="PReLU")
    assert rel_err(r.numpy().reshape(res.shape), res) <= TOL
    xe = O.conv_norm_act(res, O._sub(BLK, "projection"))
    assert rel_err(y.numpy().reshape(xe.shape), xe) <= TOL
    # with a second addend: the block input of a later application is out + a1 (refinement_module.py:58-60)
    a1 = rand((2, 256, T, F), 13)
    (r2, _), _ = R.gateway_proj(R.EXACT, _flat(x), _flat(a1), gw, gb, slope, wp, bp)
    assert rel_err(r2.numpy().reshape(res.shape), O.conv_norm_act(x + a1, O._sub(BLK, "gateway"), groups=256, act="PReLU")) <= TOL
    ex = rand((2, 64, T, F), 14)
    w1, b1 = _w(BLK, "residual_conv")
    (o,), _ = R.residual(R.EXACT, _flat(ex), w1, b1, _flat(res))
    assert rel_err(o.numpy().reshape(res.shape), O.conv_norm_act(ex, O._sub(BLK, "residual_conv")) + res) <= TOL


def test_boundary_is_residual_conv_caf_and_the_next_head():
    """Plain and with the CAF between the first two applications, Tv below and above T (refinement: rtfs_block, caf, + a1, rtfs_block)."""
    ex, res, a1 = rand((2, 64, T, F), 15), rand((2, 256, T, F), 16), rand((2, 256, T, F), 17)
    gw, gb, slope = _gate(BLK)
    wp, bp = _w(BLK, "projection")
    w1, b1 = _w(BLK, "residual_conv")
    out = O.conv_norm_act(ex, O._sub(BLK, "residual_conv")) + res
    for tv in (0, 2, 7):
        caf = None if tv == 0 else _caf_args(rand((2, 512, tv), 18 + tv), T)
        nxt = (out if tv == 0 else O.caf(out, rand((2, 512, tv), 18 + tv), CAF)) + a1
        want_r = O.conv_norm_act(nxt, O._sub(BLK, "gateway"), groups=256, act="PReLU")
        want_x = O.conv_norm_act(want_r, O._sub(BLK, "projection"))
        (r, y), _ = R.boundary(R.EXACT, _flat(ex), _flat(res), _flat(a1), w1, b1, gw, gb, slope, wp, bp, caf)
        assert rel_err(r.numpy().reshape(want_r.shape), want_r) <= TOL, tv
        assert rel_err(y.numpy().reshape(want_x.shape), want_x) <= TOL, tv
        if caf is not None:
            (r2, _), _ = R.gateway_proj(R.EXACT, _flat(out), _flat(a1), gw, gb, slope, wp, bp, caf)
            assert rel_err(r2.numpy().reshape(want_r.shape), want_r) <= TOL, tv


def test_s3_and_taps_are_the_mask_and_the_decoder():
    refined, a0 = rand((2, 256, T, F), 30), rand((2, 256, T, F), 31)
    p = O._sub(SD, "mask_generator")
    w, b = p["mask_generator.1.full_layer.2.weight"].reshape(256, 256), p["mask_generator.1.full_layer.2.bias"]
    slope = float(np.asarray(p["mask_generator.0.weight"]).reshape(-1)[0])
    sep = O.s3_mask(refined, a0, p)
    (y,), _ = R.s3(R.EXACT, _flat(refined), slope, w, b, _flat(a0))
    assert rel_err(y.numpy().reshape(a0.shape), sep[:, 0]) <= TOL
    # the 18 tap maps, shifted and added, are ConvTranspose2d(256 -> 2, 3x3, stride 1, padding 1): tap = o * 9 + kt * 3 + kf
    dw = O._sub(SD, "decoder")["decoder.weight"]
    wt = np.zeros((32, 256), np.float32)
    wt[:18] = dw.reshape(256, 18).T
    (z,), _ = R.s3_taps(R.EXACT, _flat(refined), slope, w, b, _flat(a0), wt, 18)
    z = z.numpy().reshape(2, 2, 3, 3, T, F)
    zp = np.pad(z, [(0, 0)] * 4 + [(1, 1), (1, 1)])
    y2 = sum(zp[:, :, kt, kf, 2 - kt:2 - kt + T, 2 - kf:2 - kf + F] for kt in range(3) for kf in range(3))
    assert rel_err(y2, O.conv_transpose2d_s1(sep[:, 0], dw, pad=1)) <= TOL
    (z1,), _ = R.taps(R.EXACT, sep[:, 0].reshape(2, 256, P), wt, 18)
    assert rel_err(z1.numpy().reshape(z.shape), z) <= TOL


def test_other_arithmetics_and_the_error_measure():
    """F32 and the f16x3 emulation compute the same thing to float32 accuracy (their errors set the sweep's bars, so a broken emulation would
    loosen them); the emulation without its lo.hi product is visibly worse; err() is per element and scale-free."""
    # (x 16: an activation below 2^-3 loses its flushed lo part - DESIGN.md, "Range" - which at unit scale IS the emulation's error, 1.5e-5)
    x = rand((1, 64, 130), 40, 16.0)
    res = rand((1, 256, 130), 41, 16.0)
    w1, b1 = _w(BLK, "residual_conv")
    (ref,), (sc,) = R.residual(R.EXACT, x, w1, b1, res)
    e32 = R.err(R.residual(R.F32, x, w1, b1, res)[0][0], ref, sc)
    e16 = R.err(R.residual(R.F16X3, x, w1, b1, res)[0][0], ref, sc)
    assert 0 < e32 < 2e-6 and 0 < e16 < 2e-6, (e32, e16)
    half = (torch.matmul(R.t64(w1).float().mul(256).half().float(), R.t64(x).float().half().float()) / 256 + R.t64(b1).float().reshape(1, -1, 1)
            + R.t64(res).float())
    assert R.err(half, ref, sc) > 20 * e16  # hi.hi alone: the low parts matter to the measure
    bad = ref.clone()
    k = int(sc.reshape(-1).argmin())
    bad.reshape(-1)[k] += 1e-3 * sc.reshape(-1)[k]
    assert abs(R.err(bad, ref, sc) - 1e-3) < 1e-9
    assert R.err(ref, ref, sc) == 0.0
    # integer data: the float64 form is the integer result
    rng = np.random.default_rng(0)
    xi, wi = rng.integers(-3, 4, (1, 64, 5)), rng.integers(-2, 3, (256, 64))
    (yi,), _ = R.residual(R.EXACT, xi, wi, np.zeros(256), np.zeros((1, 256, 5)))
    assert np.array_equal(yi.numpy(), np.einsum("oc,bcp->bop", wi, xi).astype(np.float64))
    (y3,), _ = R.residual(R.F16X3, xi, wi, np.zeros(256), np.zeros((1, 256, 5)))
    assert np.array_equal(y3.double().numpy(), yi.numpy())


def test_a0_rebuild_is_the_encoder_conv():
    """enc_a0 (18 taps per pixel as a GEMM) against the encoder's Conv2d of stft_encoder, at T = 1 (no row above or below) and T = 3."""
    pe = O._sub(SD, "encoder")
    for n in (256, 512):
        wav = rand((2, n), 50 + n, 0.07)
        a0, spec = O.stft_encoder(wav, pe)
        (y,), _ = R.enc_a0(R.EXACT, spec, pe["conv.full_layer.2.weight"].reshape(256, 18))
        e = rel_err(y.numpy().reshape(a0.shape), a0)
        assert e <= TOL, (n, e)
    # the fused head and tail are compositions of pieces tied above: a0 -> bottleneck -> gateway -> projection; residual conv -> mask -> taps
    spec = rand((2, 2, 2, 129), 60)
    wenc = pe["conv.full_layer.2.weight"].reshape(256, 18)
    pb = O._sub(SD, "audio_bottleneck")
    gw, gb, slope = _gate(BLK)
    wp, bp = _w(BLK, "projection")
    (a1, r, y), _ = R.bn_head(R.EXACT, spec, wenc, pb["full_layer.0.norm.weight"], pb["full_layer.0.norm.bias"],
                              pb["full_layer.2.weight"].reshape(256, 256), pb["full_layer.2.bias"], gw, gb, slope, wp, bp)
    a0 = O.conv2d_dense_same(spec, pe["conv.full_layer.2.weight"])
    want = O.conv_norm_act(a0, pb, pre_norm="gLN", pre_act="ReLU")
    assert rel_err(a1.numpy().reshape(want.shape), want) <= TOL
    wr = O.conv_norm_act(want, O._sub(BLK, "gateway"), groups=256, act="PReLU")
    assert rel_err(r.numpy().reshape(wr.shape), wr) <= TOL
    assert rel_err(y.numpy().reshape(2, 64, 2, 129), O.conv_norm_act(wr, O._sub(BLK, "projection"))) <= TOL
    # tail, two targets of mixture 1 and one of mixture 0
    pm = O._sub(SD, "mask_generator")
    ex, res = rand((3, 64, 2, 129), 61), rand((3, 256, 2, 129), 62)
    w1, b1 = _w(BLK, "residual_conv")
    dw = O._sub(SD, "decoder")["decoder.weight"]
    wt = np.zeros((32, 256), np.float32)
    wt[:18] = dw.reshape(256, 18).T
    mix = [1, 1, 0]
    (z,), _ = R.tail(R.EXACT, _flat(ex), _flat(res), spec, wenc, w1, b1, float(np.asarray(pm["mask_generator.0.weight"]).reshape(-1)[0]),
                     pm["mask_generator.1.full_layer.2.weight"].reshape(256, 256), pm["mask_generator.1.full_layer.2.bias"], wt, 18, mix=mix)
    refined = O.conv_norm_act(ex, O._sub(BLK, "residual_conv")) + res
    sep = O.s3_mask(refined, a0[mix], pm)[:, 0]
    (z1,), _ = R.taps(R.EXACT, sep.reshape(3, 256, 258), wt, 18)
    assert rel_err(z.numpy(), z1.numpy()) <= TOL


def test_emulation_error_is_bounded():
    """The sweep's float bars are ten times the f16x3 emulation's error, capped at 1e-5: an emulation that came out inaccurate would loosen
    them silently.  At the sweep's data scale (x 16) the emulation must stay below 1e-6 for every single-GEMM and boundary op - four times the
    2^-22 of the dropped lo.lo product, which leaves room for float32 accumulation over K <= 256 - and below 4e-6 where a0 is rebuilt first
    (|a0| is several times smaller than |W| @ |patch|, and that error rides through the mask product into the taps)."""
    rng = np.random.default_rng(3)
    n = lambda *s: (16 * rng.standard_normal(s)).astype(np.float32)
    wgt = lambda o, c: (rng.standard_normal((o, c)) / np.sqrt(c)).astype(np.float32)
    P = 130
    gw, gb = (1 + 0.3 * rng.standard_normal(256)).astype(np.float32), rng.standard_normal(256).astype(np.float32)
    b256, b64 = rng.standard_normal(256).astype(np.float32), rng.standard_normal(64).astype(np.float32)
    def worst(fn, *a, **k):
        refs, scales = fn(R.EXACT, *a)
        return max(R.err(e, r, s) for e, r, s in zip(fn(R.F16X3, *a, **k)[0], refs, scales))
    wt = np.zeros((32, 256), np.float32)
    wt[:18] = wgt(18, 256)
    spec, wenc = n(2, 2, 2, 65), (rng.standard_normal((256, 18)) / (16 * np.sqrt(18))).astype(np.float32)
    a0 = R.enc_a0(R.EXACT, spec, wenc)[0][0]
    esc = R.rms_pow2(R.stats(a0).numpy(), 1.0 / (256 * P))
    got = {
        "audio_bn": worst(R.audio_bn, n(2, 256, P) + 3, 16 * gw, 16 * gb, wgt(256, 256), b256),
        "gateway_proj": worst(R.gateway_proj, n(2, 256, P), n(2, 256, P), gw, gb, 0.25, wgt(64, 256), b64),
        "residual": worst(R.residual, n(2, 64, P), wgt(256, 64), b256, n(2, 256, P)),
        "boundary": worst(R.boundary, n(2, 64, P), n(2, 256, P), n(2, 256, P), wgt(256, 64), b256, gw, gb, 0.25, wgt(64, 256), b64),
        "s3": worst(R.s3, n(2, 256, P), 0.25, wgt(256, 256), b256, n(2, 256, P)),
        "s3_taps": worst(R.s3_taps, n(2, 256, P), 0.25, wgt(256, 256), b256, n(2, 256, P), wt, 18),
        "bn_head": worst(R.bn_head, spec, wenc, 16 * gw, 16 * gb, wgt(256, 256), b256, gw, gb, 0.25, wgt(64, 256), b64, esc=esc),
        "tail": worst(R.tail, n(2, 64, P), n(2, 256, P), spec, wenc, wgt(256, 64), b256, 0.25, wgt(256, 256), b256, wt, 18, esc=esc),
    }
    print(got)
    for k, v in got.items():
        assert 0 < v < (4e-6 if k == "tail" else 1e-6), (k, v)
