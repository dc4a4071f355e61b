"""CPU: ties tests/attn_reference.py (the float64 restatement tests/test_hip_attn_edges.py holds the attention kernels to) to
oracle/rtfs_oracle.py::mhsa2d on the oracle's own state dict, and measures the f16x3 emulation against it on the sweep's float-tier
inputs: ten times these values (capped at 1e-5) are the sweep's bars, so an emulation that came out inaccurate would loosen them."""
import numpy as np
import torch

from oracle import rtfs_oracle as O
from oracle.params import make_state_dict
from tests import attn_reference as A
from tests.util import rand, rel_err, spec_R4

TOL = 2e-5
SD = make_state_dict(spec_R4(), 0)
ATT = O._sub(O._sub(SD, "refinement_module.audio_net.blocks"), "globalatt.2")


def test_three_stages_compose_to_the_oracle():
    P = A.params_of(ATT)
    for B, T in ((2, 5), (1, 33)):
        x = rand((B, 64, T, 64), 70 + T)
        y = A.mhsa(A.EXACT, x, P)
        e = rel_err(y.numpy(), O.mhsa2d(x, ATT))
        assert e <= TOL, (B, T, e)


def test_group_table_and_layouts():
    """Q / K / V land head-major with the module's own slope: each module's output must equal the oracle's ConvActNorm of that module."""
    P = A.params_of(ATT)
    x = rand((2, 64, 3, 64), 71)
    (q, k, v), dens = A.qkv(A.EXACT, x, P["qkv_w"], P["qkv_b"], P["qkv_slope"], P["qkv_gamma"], P["qkv_beta"])
    for name, got in (("Queries", q), ("Keys", k), ("Values", v)):
        for h in range(4):
            want = O._conv_act_norm(x, O._sub(ATT, f"{name}.{h}")).transpose(0, 2, 1, 3).reshape(2, 3, -1)
            assert rel_err(got[:, h].numpy(), want) <= TOL, (name, h)
    assert all(float(d.min()) > 0 for d in dens)


def test_emulation_error_per_stage():
    """The f16x3 emulation against float64 on the float-tier inputs of the sweep, the sweep's own measure.  Every stage must stay below
    1e-6: four times the 2^-22 of the dropped lo.lo product, which leaves room for float32 accumulation over K <= 512 and the float32
    LayerNorm / softmax - then ten times the value is below the 1e-5 cap and the bar really is set by the emulation.  (With V split
    unscaled the core came out at 3.8e-6: a V element below 2^-2 lost its flushed low part.  V is stored times 64 since.)"""
    rng = np.random.default_rng(5)
    got = {}
    p = A.row_params(rng, 96)
    x = A.row_input(rng, 3, 5)
    refs, dens = A.qkv(A.EXACT, x, **p)
    emus, _ = A.qkv(A.F16X3, x, **p)
    for n, e, r, d in zip("qkv", emus, refs, dens):
        got[f"qkv {n}"] = A.err(e, r, d)
    p = A.row_params(rng, 64)
    o, res = A.row_input(rng, 3, 5), rng.standard_normal((3, 64, 5, 64)).astype(np.float32)
    (r,), (d,) = A.proj(A.EXACT, o, res, **p)
    got["proj"] = A.err(A.proj(A.F16X3, o, res, **p)[0][0], r, d)
    for T in (33, 257):
        q, k, v = A.core_inputs(rng, 1, T)
        (r,), (d,) = A.core(A.EXACT, q, k, v, A.CORE_SCALE)
        got[f"core T{T}"] = A.err(A.core(A.F16X3, q, k, v, A.CORE_SCALE)[0][0], r, d)
        p_ = torch.softmax(torch.matmul(A.t64(q), A.t64(k).transpose(-1, -2)) * A.CORE_SCALE, -1)
        top = float(p_.amax(-1).median())
        assert 2.0 / T < top < 0.9, (T, top)  # neither flat nor one-hot
    print("f16x3 emulation, worst per stage:", {k: f"{v:.3e}" for k, v in got.items()})
    for k, v in got.items():
        assert 0 < v < 1e-6, (k, v)


def test_measure_and_exact_tiers():
    """err() is per element; on the selection tier's data (K = +-1, Q = 16 K[pi], integer V) both arithmetics return V[pi] exactly; with Q = 0
    the output is the mean of the V rows."""
    rng = np.random.default_rng(6)
    T = 33
    k = rng.choice([-1.0, 1.0], (1, 4, T, 256)).astype(np.float32)
    pi = np.stack([rng.permutation(T) for _ in range(4)])
    q = 16 * np.stack([k[0, h, pi[h]] for h in range(4)])[None]
    v = rng.integers(-8, 9, (1, 4, T, 1024)).astype(np.float32)
    want = np.stack([v[0, h, pi[h]] for h in range(4)]).reshape(4, T, 16, 64).transpose(0, 2, 1, 3).reshape(1, 64, T, 64)
    s = np.einsum("bhqe,bhke->bhqk", q.astype(np.float64), k.astype(np.float64)) / 16
    top = np.sort(s, -1)
    assert (top[..., -1] == 256).all() and (top[..., -1] - top[..., -2]).min() >= 110  # expf of the runner-up is 0 in float32, not in float64
    (o,), _ = A.core(A.F16X3, q, k, v)
    assert np.array_equal(o.numpy(), want)
    (o,), _ = A.core(A.EXACT, q, k, v)
    assert np.abs(o.numpy() - want).max() < 1e-40
    (o,), (d,) = A.core(A.EXACT, np.zeros_like(q), k, v)
    assert np.allclose(o.numpy(), np.broadcast_to(v.mean(2, keepdims=True), v.shape).reshape(4, T, 16, 64).transpose(0, 2, 1, 3).reshape(1, 64, T, 64))
    bad = o.clone()
    i = int(d.reshape(-1).argmin())
    bad.reshape(-1)[i] += 1e-3 * d.reshape(-1)[i]
    assert abs(A.err(bad, o, d) - 1e-3) < 1e-9 and A.err(o, o, d) == 0.0
