"""CPU: ties tests/dw_reference.py (the float64 restatement tests/test_hip_dw_edges.py holds the depthwise kernels to) to
oracle/rtfs_oracle.py, which tests/test_oracle_golden.py pins against the reference project's own vectors.  Bar: that file's 2e-5."""
import numpy as np
import torch

from oracle import rtfs_oracle as O
from oracle.params import make_state_dict
from tests import dw_reference as D
from tests.util import rand, rel_err, spec_R4

TOL = 2e-5
SD = make_state_dict(spec_R4(), 0)
BLK = O._sub(SD, "refinement_module.audio_net.blocks")


def _cna(p, name):
    """(weight, bias or None, (gamma, beta)) of the ConvNormAct ``name``."""
    q = O._sub(p, name)
    return q["full_layer.2.weight"], q.get("full_layer.2.bias"), (q["full_layer.3.norm.weight"], q["full_layer.3.norm.bias"])


def _tfar_up(loc, glo, p):
    """InjectionMultiSum with a larger local map as "three plain convs + apply"."""
    lw, _, lgb = _cna(p, "local_embedding")
    ew, _, egb = _cna(p, "global_embedding")
    gw, _, ggb = _cna(p, "global_gate")
    x, g = D.t64(loc), D.t64(glo)
    E, G = D.conv_s1(g, ew), D.conv_s1(g, gw)
    return D.apply(x, lw, D.stats(D.conv_s1(x, lw)), lgb, G, D.stats(G), ggb, E, D.stats(E), egb)


def test_three_convs_and_apply_are_injection_multi_sum():
    """The tests/test_hip_parity.py::test_tfar inputs: (8, 64) -> (17, 129) through up(), and the same-size form through combine()."""
    glo = rand((2, 64, 8, 64), 105)
    loc = rand((2, 64, 17, 129), 104)
    p = O._sub(BLK, "fusion_layers.0")
    e = rel_err(_tfar_up(loc, glo, p).numpy(), O.injection_multi_sum(loc, glo, p))
    assert e <= TOL, e
    loc = rand((2, 64, 8, 64), 106)
    p = O._sub(BLK, "fusion_layers.1")
    lw, _, lgb = _cna(p, "local_embedding")
    ew, _, egb = _cna(p, "global_embedding")
    gw, _, ggb = _cna(p, "global_gate")
    L, E, G = D.conv_s1(D.t64(loc), lw), D.conv_s1(D.t64(glo), ew), D.conv_s1(D.t64(glo), gw)
    y = D.combine(L, D.stats(L), lgb, G, D.stats(G), ggb, E, D.stats(E), egb)
    e = rel_err(y.numpy(), O.injection_multi_sum(loc, glo, p))
    assert e <= TOL, e


def test_departing_pair_goes_through_the_float32_index():
    """(14, 26) -> (46, 44): the integer quotient is not torch's index there (tests/nearest_cases.py); up() must follow the oracle."""
    glo, loc = rand((1, 64, 14, 26), 7), rand((1, 64, 46, 44), 8)
    p = O._sub(BLK, "fusion_layers.0")
    e = rel_err(_tfar_up(loc, glo, p).numpy(), O.injection_multi_sum(loc, glo, p))
    assert e <= TOL, e


def test_stride2_pool_and_g_form_are_the_block_internals():
    """d0, d1 and g_in of O.rtfs_block from "stride-1 conv + fold", "stride-2 + pool" and g_form."""
    x = rand((1, 256, 17, 129), 115)
    _, ints = O.rtfs_block(x, BLK, return_internals=True)
    w0, b0, gb0 = _cna(BLK, "downsample_layers.0")
    w1, b1, gb1 = _cna(BLK, "downsample_layers.1")
    c0 = D.conv_s1(D.t64(ints["x_enc"]), w0, b0)
    d0 = D.fold(c0, D.stats(c0), *gb0)
    assert rel_err(d0.numpy(), ints["d0"]) <= TOL
    c1, p0 = D.s2_pool(d0, w1, b1, (17 // 2, 129 // 2))
    assert tuple(c1.shape) == ints["d1"].shape
    assert rel_err(D.fold(c1, D.stats(c1), *gb1).numpy(), ints["d1"]) <= TOL
    g = D.g_form(p0, c1, D.stats(c1), gb1)
    e = rel_err(g.numpy(), ints["g_in"])
    assert e <= TOL, e


def test_dtypes_and_integer_form():
    """The float32 run keeps float32, and the int64 form equals the float64 one on integer data (it is the exact reference)."""
    rng = np.random.default_rng(0)
    x = torch.as_tensor(rng.integers(-2, 3, (2, 4, 5, 7)))
    w = torch.as_tensor(rng.integers(-2, 3, (4, 16)))
    b = torch.as_tensor(rng.integers(-1, 2, (4,)))
    for f in (D.conv_s1, D.conv_s2):
        yi = f(x, w, b)
        assert yi.dtype == torch.int64 and torch.equal(yi.double(), f(x.double(), w.double(), b.double()))
        assert f(x.float(), w.float(), b.float()).dtype == torch.float32
    # one hand-checked tap: output (0, 0) of the stride-1 form meets x[0:3, 0:3] under w[1:, 1:]
    want = int((x[0, 0, :3, :3] * w[0].reshape(4, 4)[1:, 1:]).sum() + b[0])
    assert int(D.conv_s1(x, w, b)[0, 0, 0, 0]) == want
    want = int((x[0, 0, 3:5, 5:7] * w[0].reshape(4, 4)[:2, :2]).sum() + b[0])  # (4, 6): rows 3..4, columns 5..6 remain
    assert int(D.conv_s1(x, w, b)[0, 0, 4, 6]) == want
